// tests/native_flow/flow_asan_main.cpp — TEST ONLY: a stand-alone driver for the flow handler's
// decoder and manager under -fsanitize=address,undefined (built by tests/test_flow_host.py together
// with flow_harness.cpp, pv_flow.cpp and pv_dhcp.cpp): every file named on the command line (classic
// pcap records, linktype in the first argument) through decode, replay and both JSON reads, with
// every group enabled and with the defaults, on any port and on port 2055.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

struct Row {
    uint16_t last, first;
    uint32_t protocol;
    const char *name;
};

extern "C" {
void *fl_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate, uint32_t groups, uint32_t topn, uint32_t pct,
             const uint16_t *ports, uint32_t nports, const Row *rows, uint32_t nrows);
void fl_free(void *h);
void fl_feed(void *hp, const uint8_t *recs, size_t bytes);
void fl_set_end(void *h, int64_t sec, int64_t nsec);
char *fl_json(void *hp, uint32_t period, int merged);
void fl_free_str(char *s);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: flow_asan LINKTYPE FILE...\n"); return 2; }
    const uint32_t linktype = (uint32_t)atoi(argv[1]);
    const Row rows[3] = {{23, 23, 6, "telnet"}, {520, 520, 17, "router"}, {6063, 6000, 6, "x11"}};
    const uint16_t port = 2055;
    size_t total = 0;
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        std::vector<uint8_t> recs((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (int v = 0; v < 4; v++) {
            void *h = fl_new(linktype, 0, 3, v & 1 ? 50 : 100, v & 2 ? 0x7ff : 0x7f, 10, 0, &port, v & 1, rows, v & 2 ? 3 : 0);
            fl_feed(h, recs.data(), recs.size());
            fl_set_end(h, 0x7fffffff, 0);
            for (int merged = 0; merged < 2; merged++) {
                char *j = fl_json(h, merged ? 3 : 0, merged);
                total += strlen(j);
                fl_free_str(j);
            }
            fl_free(h);
        }
    }
    printf("read %zu JSON bytes\n", total);
    return 0;
}
