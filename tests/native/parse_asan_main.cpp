// tests/native/parse_asan_main.cpp — TEST ONLY: a stand-alone driver of parse_record (pv_parse.h)
// for a sanitizer build (tests/test_parse_fuzz.py compiles it with parse_harness.cpp under
// -DPV_PARSE_BOUNDED -fsanitize=address,undefined). The corpus file holds groups:
//   u32 linktype, u32 n4, n4 x (u32 s_addr, u32 cidr), u32 n6, n6 x (16 bytes, u32 cidr),
//   u64 bytes of records, then the classic-pcap records themselves.
// Each record is parsed from a heap copy of exactly 16 + caplen bytes, once for each of two values
// standing in for the bytes behind it (see BAcc in parse_harness.cpp): a byte read past the copy
// is a sanitizer report, and rows that differ between the two runs mean the result depends on what
// follows the record. Exits 0 when neither happens.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

extern "C" void h_parse_bounded(const uint8_t *rec, uint64_t size, uint8_t fill, uint32_t linktype, uint32_t n4,
                                const uint32_t *v4_addr, const uint32_t *v4_cidr, uint32_t n6, const uint8_t *v6_addr,
                                const uint32_t *v6_cidr, int64_t *row);

struct Reader {
    const std::vector<uint8_t> &b;
    size_t pos = 0;
    bool need(size_t n) const { return pos + n <= b.size(); }
    template <class T> T get()
    {
        T v;
        if (!need(sizeof v)) { fprintf(stderr, "corpus file ends inside a group header\n"); exit(2); }
        memcpy(&v, b.data() + pos, sizeof v);
        pos += sizeof v;
        return v;
    }
};

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: parse_asan FILE...\n"); return 2; }
    size_t records = 0, groups = 0, with_l4 = 0;
    for (int i = 1; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        Reader r{buf};
        while (r.pos < buf.size()) {
            const uint32_t linktype = r.get<uint32_t>();
            std::vector<uint32_t> a4, c4, c6;
            std::vector<uint8_t> a6;
            const uint32_t n4 = r.get<uint32_t>();
            for (uint32_t k = 0; k < n4; k++) { a4.push_back(r.get<uint32_t>()); c4.push_back(r.get<uint32_t>()); }
            const uint32_t n6 = r.get<uint32_t>();
            for (uint32_t k = 0; k < n6; k++) {
                for (int j = 0; j < 16; j++) a6.push_back(r.get<uint8_t>());
                c6.push_back(r.get<uint32_t>());
            }
            const uint64_t bytes = r.get<uint64_t>();
            if (!r.need(bytes)) { fprintf(stderr, "%s: a group runs past the end\n", argv[i]); return 2; }
            const size_t end = r.pos + bytes;
            while (r.pos + 16 <= end) {
                uint32_t hd[4];
                memcpy(hd, buf.data() + r.pos, 16);
                const size_t size = 16 + (size_t)hd[2];
                if (r.pos + size > end) { fprintf(stderr, "%s: a record runs past its group\n", argv[i]); return 2; }
                uint8_t *copy = (uint8_t *)malloc(size); // exactly the record: nothing readable behind it
                memcpy(copy, buf.data() + r.pos, size);
                int64_t row[2][10];
                for (int k = 0; k < 2; k++)
                    h_parse_bounded(copy, size, k ? 0xff : 0x00, linktype, n4, a4.data(), c4.data(), n6, a6.data(), c6.data(),
                                    row[k]);
                free(copy);
                if (memcmp(row[0], row[1], sizeof row[0]) != 0) {
                    fprintf(stderr, "%s: record at byte %zu (caplen %u, linktype %u): the row depends on the bytes behind it\n",
                            argv[i], r.pos, hd[2], linktype);
                    return 3;
                }
                with_l4 += row[0][1] != 0;
                records++;
                r.pos += size;
            }
            r.pos = end;
            groups++;
        }
    }
    printf("%zu records in %zu groups, %zu with an L4 layer\n", records, groups, with_l4);
    return 0;
}
