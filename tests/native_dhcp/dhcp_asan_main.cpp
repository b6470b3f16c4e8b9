// tests/native_dhcp/dhcp_asan_main.cpp — TEST ONLY: a stand-alone driver for the DHCP decoder
// and manager under -fsanitize=address,undefined (built by tests/test_dhcp_host.py together
// with dhcp_harness.cpp and pv_dhcp.cpp): every corpus file named on the command line (classic
// pcap records, linktype in the first argument) through decode, replay and both JSON reads.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

extern "C" {
void *dh_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate, uint32_t ttl_ms, uint32_t topn, uint32_t pct);
void dh_free(void *h);
void dh_feed(void *hp, const uint8_t *recs, size_t bytes);
void dh_set_end(void *h, int64_t sec, int64_t nsec);
char *dh_json(void *hp, uint32_t period, int merged);
void dh_free_str(char *s);
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: dhcp_asan LINKTYPE FILE...\n"); return 2; }
    const uint32_t linktype = (uint32_t)atoi(argv[1]);
    size_t total = 0;
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        std::vector<uint8_t> recs((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        for (uint32_t rate : {100u, 50u}) {
            void *h = dh_new(linktype, 0, 3, rate, 5000, 10, 0);
            dh_feed(h, recs.data(), recs.size());
            dh_set_end(h, 0x7fffffff, 0);
            for (int merged = 0; merged < 2; merged++) {
                char *j = dh_json(h, merged ? 3 : 0, merged);
                total += strlen(j);
                dh_free_str(j);
            }
            dh_free(h);
        }
    }
    printf("read %zu JSON bytes\n", total);
    return 0;
}
