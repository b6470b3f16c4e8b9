// tests/native_bpf/bpf_asan_main.cpp — TEST ONLY: a stand-alone driver for the classic-BPF checker
// and host machine (pv_bpf.cpp) under -fsanitize=address,undefined, built by tests/test_bpf_fuzz.py
// into a temporary directory.
//
//   bpf_asan PROGRAMS RECORDS
//
// PROGRAMS: a run of { u32 run, u32 n, n x struct sock_filter }. Every program goes through
// pv_bpf_validate, from a heap block of exactly n instructions. One with run != 0 must validate;
// it then runs on every record of RECORDS (classic-pcap records, host order), each frame in a heap
// block of exactly caplen bytes, and filters the whole blob through pv_bpf_filter_records from and
// into blocks of exactly the blob's size. Prints the counts and the sum of all answers, which the
// test compares with the Python restatement's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdint.h>
#include <vector>

#include "../../include/pvgpu.h"

static std::vector<uint8_t> slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Frame {
    uint8_t *p; // exactly caplen bytes
    uint32_t caplen, wirelen;
};

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: bpf_asan PROGRAMS RECORDS\n"); return 2; }
    const std::vector<uint8_t> progs = slurp(argv[1]), recs = slurp(argv[2]);
    std::vector<Frame> frames;
    for (size_t pos = 0; pos + 16 <= recs.size();) {
        uint32_t hd[4];
        memcpy(hd, recs.data() + pos, 16);
        if (pos + 16 + (size_t)hd[2] > recs.size()) { fprintf(stderr, "a record runs past the end\n"); return 2; }
        Frame f{(uint8_t *)malloc(hd[2] ? hd[2] : 1), hd[2], hd[3]};
        if (hd[2]) memcpy(f.p, recs.data() + pos + 16, hd[2]);
        else { free(f.p); f.p = nullptr; } // no byte of an empty capture may be read at all
        frames.push_back(f);
        pos += 16 + (size_t)hd[2];
    }
    uint8_t *in = (uint8_t *)malloc(recs.size() ? recs.size() : 1), *out = (uint8_t *)malloc(recs.size() ? recs.size() : 1);
    if (!recs.empty()) memcpy(in, recs.data(), recs.size());
    size_t n_progs = 0, n_valid = 0, n_run = 0;
    uint64_t sum = 0, kept_records = 0, kept_bytes = 0;
    for (size_t pos = 0; pos + 8 <= progs.size();) {
        uint32_t hd[2];
        memcpy(hd, progs.data() + pos, 8);
        const size_t bytes = (size_t)hd[1] * sizeof(pv_bpf_insn);
        if (pos + 8 + bytes > progs.size()) { fprintf(stderr, "a program runs past the end\n"); return 2; }
        pv_bpf_insn *p = hd[1] ? (pv_bpf_insn *)malloc(bytes) : nullptr;
        if (hd[1]) memcpy(p, progs.data() + pos + 8, bytes);
        pos += 8 + bytes;
        n_progs++;
        const int rc = pv_bpf_validate(p, hd[1]);
        n_valid += rc == 0;
        if (hd[0]) {
            if (rc) { fprintf(stderr, "program %zu: marked to run, refused by the checker\n", n_progs - 1); return 1; }
            for (const Frame &f : frames) sum += pv_bpf_run(p, f.p, f.wirelen, f.caplen);
            size_t ob = 0;
            uint64_t k = 0;
            if (pv_bpf_filter_records(p, hd[1], in, recs.size(), out, &ob, &k)) { fprintf(stderr, "filter_records failed\n"); return 1; }
            kept_records += k;
            kept_bytes += ob;
            n_run++;
        }
        free(p);
    }
    for (Frame &f : frames) free(f.p);
    free(in);
    free(out);
    printf("%zu programs, %zu valid, %zu run on %zu records: sum %llu, kept %llu records, %llu bytes\n", n_progs, n_valid, n_run,
           frames.size(), (unsigned long long)sum, (unsigned long long)kept_records, (unsigned long long)kept_bytes);
    return 0;
}
