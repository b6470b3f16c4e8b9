// tests/native/dns_asan_main.cpp — TEST ONLY: a stand-alone driver of the DNS decode (pv_parse.h:
// name_len_l1, name_emit, name_stats_fast, dns_parse, dns_dnssec, dns_first_additional, dns_ecs)
// for a sanitizer build (tests/test_decoder_fuzz.py compiles it with parse_harness.cpp under
// -fsanitize=address,undefined). The corpus file is a sequence of (u32 length, message bytes).
//   usage: dns_asan PAD FILE...
// Each message is decoded from a heap copy of exactly length + PAD bytes (PAD: the measured bound
// of the decode's reads past the message, which the record blob's padding covers on the device),
// once with the PAD bytes 0x00 and once 0xff: a read past the copy is a sanitizer report, and
// results that differ between the two mean the decode depends on what follows the message. Exits 0
// when neither happens.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

#define PV_DNS_ALL_VALS 15
extern "C" void h_dns_all(const uint8_t *msg, uint32_t len, uint64_t *v, char *name, uint32_t *name_n);

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: dns_asan PAD FILE...\n"); return 2; }
    const size_t pad = (size_t)strtoul(argv[1], nullptr, 10);
    size_t messages = 0, named = 0;
    std::vector<char> name[2] = {std::vector<char>(4096), std::vector<char>(4096)};
    for (int i = 2; i < argc; i++) {
        std::ifstream f(argv[i], std::ios::binary);
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[i]); return 2; }
        const std::vector<uint8_t> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        size_t pos = 0;
        while (pos < buf.size()) {
            uint32_t len;
            if (pos + 4 > buf.size()) { fprintf(stderr, "%s ends inside a length\n", argv[i]); return 2; }
            memcpy(&len, buf.data() + pos, 4);
            pos += 4;
            if (pos + len > buf.size()) { fprintf(stderr, "%s: a message runs past the end\n", argv[i]); return 2; }
            uint8_t *copy = (uint8_t *)malloc(len + pad); // nothing readable behind it
            memcpy(copy, buf.data() + pos, len);
            uint64_t v[2][PV_DNS_ALL_VALS];
            uint32_t n[2];
            for (int k = 0; k < 2; k++) {
                memset(copy + len, k ? 0xff : 0x00, pad);
                h_dns_all(copy, len, v[k], name[k].data(), &n[k]);
            }
            free(copy);
            if (memcmp(v[0], v[1], sizeof v[0]) != 0 || n[0] != n[1] || memcmp(name[0].data(), name[1].data(), n[0]) != 0) {
                fprintf(stderr, "%s: message at byte %zu (length %u): the decode depends on the bytes behind it\n", argv[i], pos,
                        len);
                return 3;
            }
            named += n[0] != 0;
            messages++;
            pos += len;
        }
    }
    printf("%zu messages, %zu with a name\n", messages, named);
    return 0;
}
