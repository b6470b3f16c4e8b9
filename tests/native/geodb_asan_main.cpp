// SPDX-License-Identifier: MPL-2.0
//
// Stand-alone driver of the GeoIP reader for a sanitizer build (tests/test_geodb.py compiles it
// with pv_geodb.cpp under -fsanitize=address,undefined): opens each file given, as both kinds,
// looks a spread of addresses up, then does the same over seeded byte mutations and truncations of
// it. Exits 0 when the reader neither crashes nor reads out of bounds; a refused file is fine.
#include "../../include/pvgpu.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static uint64_t rng_state = 1;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static int opened = 0, refused = 0;

static void exercise(const std::vector<uint8_t> &buf)
{
    // an exact-size heap copy, so a read past the end is a report
    uint8_t *copy = (uint8_t *)malloc(buf.size() ? buf.size() : 1);
    memcpy(copy, buf.data(), buf.size());
    for (uint32_t kind = 0; kind < 2; kind++) {
        pv_geodb *db = nullptr;
        if (pv_geodb_open(copy, buf.size(), kind, &db) != PV_OK) {
            if (!pv_geodb_last_error()[0]) { fprintf(stderr, "refusal without a message\n"); exit(2); }
            refused++;
            continue;
        }
        opened++;
        const uint32_t n = pv_geodb_entries(db);
        for (uint32_t id = 0; id < n; id++) {
            const char *a, *b, *c;
            if (pv_geodb_entry(db, id, &a, &b, &c) != PV_OK || !a || !b || !c) { fprintf(stderr, "entry %u\n", id); exit(2); }
        }
        uint8_t addrs[256 * 16];
        uint32_t ids[256];
        for (uint32_t len : {4u, 16u}) {
            for (size_t i = 0; i < sizeof addrs; i++) addrs[i] = (uint8_t)rnd();
            memset(addrs, 0, 16);
            if (pv_geodb_lookup(db, addrs, 256, len, ids) != PV_OK) { fprintf(stderr, "lookup\n"); exit(2); }
            for (uint32_t i = 0; i < 256; i++)
                if (ids[i] >= n) { fprintf(stderr, "id %u of %u\n", ids[i], n); exit(2); }
        }
        pv_geodb_close(db);
    }
    free(copy);
}

int main(int argc, char **argv)
{
    const int mutations = argc > 1 ? atoi(argv[1]) : 0;
    for (int a = 2; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<uint8_t> buf;
        uint8_t chunk[65536];
        size_t n;
        while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
        fclose(f);
        exercise(buf);
        if (!opened) { fprintf(stderr, "%s does not open\n", argv[a]); return 2; }
        rng_state = 12345 + a;
        for (int m = 0; m < mutations; m++) {
            std::vector<uint8_t> mut = buf;
            const uint32_t flips = 1 + rnd() % 8;
            // half of the mutations hit the metadata and the end of the data section, where a
            // changed byte moves node_count, record_size or a pointer
            for (uint32_t k = 0; k < flips; k++) {
                const size_t tail = mut.size() < 2048 ? mut.size() : 2048;
                const size_t pos = (m & 1) ? mut.size() - 1 - rnd() % tail : rnd() % mut.size();
                mut[pos] = (uint8_t)rnd();
            }
            if (m % 7 == 0) mut.resize(rnd() % mut.size());
            exercise(mut);
        }
    }
    printf("opened %d refused %d\n", opened, refused);
    return 0;
}
