// tests/native_bgp/bgp_asan_main.cpp — TEST ONLY: a stand-alone driver for the BGP segment
// extraction and manager under -fsanitize=address,undefined (built by tests/test_bgp_host.py
// together with bgp_harness.cpp and pv_bgp.cpp). Every corpus file named on the command line
// holds classic pcap records (linktype in the first argument): a run of streams, each ended by a
// marker record (seconds 0xffffffff, no bytes). A stream goes through a manager of its own in
// batches of BATCH records, each record decoded from an exact-size copy of its own, then the
// end-of-capture flush and both JSON reads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

extern "C" {
void *bg_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate);
void bg_free(void *h);
void bg_set_pad(void *h, uint32_t pad);
void bg_feed(void *hp, const uint8_t *recs, size_t bytes, int eoc);
void bg_set_end(void *h, int64_t sec, int64_t nsec);
char *bg_json(void *hp, uint32_t period, int merged);
void bg_free_str(char *s);
}

static bool is_marker(const std::vector<uint8_t> &r, size_t pos)
{
    uint32_t hd[4];
    memcpy(hd, r.data() + pos, 16);
    return hd[0] == 0xffffffffu && hd[2] == 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: bgp_asan LINKTYPE BATCH FILE...\n"); return 2; }
    const uint32_t linktype = (uint32_t)atoi(argv[1]);
    const size_t batch = (size_t)atoi(argv[2]);
    size_t total = 0, streams = 0;
    for (int i = 3; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        const std::vector<uint8_t> recs((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (uint32_t rate : {100u, 50u}) {
            size_t pos = 0;
            while (pos + 16 <= recs.size()) {
                void *h = bg_new(linktype, 0, 3, rate);
                bg_set_pad(h, 0);
                while (pos + 16 <= recs.size() && !is_marker(recs, pos)) {
                    size_t end = pos;
                    for (size_t n = 0; n < batch && end + 16 <= recs.size() && !is_marker(recs, end); n++) {
                        uint32_t hd[4];
                        memcpy(hd, recs.data() + end, 16);
                        end += 16 + (size_t)hd[2];
                    }
                    if (end > recs.size()) { fprintf(stderr, "%s: a record runs past the end\n", argv[i]); return 2; }
                    const bool last = end + 16 > recs.size() || is_marker(recs, end);
                    bg_feed(h, recs.data() + pos, end - pos, last);
                    pos = end;
                }
                pos += 16; // the marker
                bg_set_end(h, 0x7fffffff, 0);
                for (int merged = 0; merged < 2; merged++) {
                    char *j = bg_json(h, merged ? 3 : 0, merged);
                    total += strlen(j);
                    bg_free_str(j);
                }
                bg_free(h);
                streams++;
            }
        }
    }
    printf("%zu streams, read %zu JSON bytes\n", streams, total);
    return 0;
}
