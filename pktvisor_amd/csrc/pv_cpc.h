// SPDX-License-Identifier: MPL-2.0
// pv_cpc.h — the CPC sketch estimators (lg_k = 11) every cardinality of the outputs is rendered
// with. Plain C++ without a HIP header, so the host managers that keep their own coupons
// (pv_flow.cpp) and the CPU test harnesses use the very code the renderer (pv_render.cpp) uses.
#pragma once
#include <algorithm>
#include <cmath>
#include <stdint.h>
#include <utility>
#include <vector>

namespace pvh {

// ICON polynomial for lg_k = 11 (3rd/datasketches/cpc/include/icon_estimator.hpp:98-102)
const double ICON11[20] = {
    0.9999186020796150265, 0.3333249054574359826, 0.126791713589799987, -0.06662487271699729652,
    -0.07335552427910230211, 0.3316370184815959909, -1.434143797561290068, 4.180260309967409604,
    -8.593906870708760692, 12.95088874800289958, -14.56876092520539956, 12.37074367531410068,
    -7.969152075707960137, 3.888774396648960074, -1.424923326506990051, 0.385084561785229984,
    -0.07435541911616409816, 0.009695363567476529554, -0.0007644375960047160388, 2.75156194717188011e-05};

inline double icon11(uint32_t c)
{
    if (c < 2) return c == 0 ? 0.0 : 1.0;
    const double k = 2048.0, dc = (double)c;
    if (dc > 5.7 * k) return 0.7940236163830469 * k * pow(2.0, dc / k);
    const double x = dc / (2.0 * k);
    double t = ICON11[19];
    for (int j = 18; j >= 0; j--) t = t * x + ICON11[j];
    const double r = dc / k;
    const double res = dc * t * (1.0 + r * r * r / 66.774757);
    return res >= dc ? res : dc;
}

// HIP estimate replayed from coupons in first-occurrence order, with the
// sparse->windowed promotion and the kxp refresh of every 8th window move
// (cpc_sketch_impl.hpp:196-380).
inline double cpc_hip(std::vector<std::pair<int64_t, uint32_t>> &firsts)
{
    std::sort(firsts.begin(), firsts.end());
    std::vector<uint64_t> rows(2048, 0);
    static double kxp_byte[256];
    static bool init = false;
    if (!init) {
        for (int b = 0; b < 256; b++) {
            double s = 0;
            for (int c = 0; c < 8; c++) if (!((b >> c) & 1)) s += ldexp(1.0, -(c + 1));
            kxp_byte[b] = s;
        }
        init = true;
    }
    double kxp = 2048.0, hip = 0;
    uint32_t C = 0;
    int w = 0;
    bool windowed = false;
    for (auto &f : firsts) {
        uint32_t row = f.second >> 6, col = f.second & 63;
        rows[row] |= 1ull << col;
        C++;
        hip += 2048.0 / kxp;
        kxp -= ldexp(1.0, -(int)(col + 1));
        if (!windowed) {
            if (((uint64_t)C << 5) >= 3ull * 2048) windowed = true;
        } else if (((uint64_t)C << 3) >= (27ull + ((uint64_t)w << 3)) * 2048) {
            w++;
            if ((w & 7) == 0) {
                double bs[8] = {0};
                for (int i = 0; i < 2048; i++) {
                    uint64_t word = rows[i];
                    for (int j = 0; j < 8; j++) { bs[j] += kxp_byte[word & 0xff]; word >>= 8; }
                }
                double tot = 0;
                for (int j = 7; j >= 0; j--) tot += ldexp(1.0, -8 * j) * bs[j];
                kxp = tot;
            }
        }
    }
    return hip;
}

} // namespace pvh
