// record_text_host_bench.cpp — how long the C++ host takes to form every sample column `GT:GQ:GL:KC` of a cohort from the
// device's record fields: pangenie::record_field_text (the ostringstream and one pg_gl_text per value that
// Graph::genotypes_records runs per record), chain after chain on T threads.  Built and run by tools/bench_record_text.py.
//
//   record_text_host_bench <fields file> <text file out> <repeats> <threads> [<threads> ...]
//
// <fields file> (little endian): u64 n_chains, then per chain u64 R, u64 n_gl, pg_call [R], u64 gl_off [R + 1], pg_gl [n_gl],
// u16 kc [R], u8 no_call [R].  A record of fewer than three values, with a deferred call or a value without text has no text
// here either (the existing finishing paths complete those).  <text file out>: the bytes of all records, chain after chain.
// Prints one JSON line: per thread count the median, min and max of <repeats> formations in ms.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "../pangenie_amd/host/graph_io.hpp"

using namespace pangenie;

struct Chain {
    RecordFields fields;
    std::vector<uint16_t> kc;
    std::vector<uint8_t> no_call, skip;
    std::string text;
};

static void form(Chain& c) {
    c.text.clear();
    const size_t R = c.fields.calls.size();
    for (size_t q = 0; q < R; ++q)
        if (!c.skip[q]) c.text += record_field_text(c.fields, q, c.kc[q], c.no_call[q] != 0);
}

int main(int argc, char** argv) {
    if (argc < 5) { std::printf("usage: record_text_host_bench <fields file> <text file out> <repeats> <threads> [<threads> ...]\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { std::printf("cannot open %s\n", argv[1]); return 1; }
    uint64_t n_chains = 0;
    in.read((char*)&n_chains, 8);
    std::vector<Chain> chains(n_chains);
    for (Chain& c : chains) {
        uint64_t R = 0, n_gl = 0;
        in.read((char*)&R, 8);
        in.read((char*)&n_gl, 8);
        std::vector<pg_call> calls(R);
        c.fields.gl_off.resize(R + 1);
        c.fields.gl.resize(n_gl);
        c.kc.resize(R);
        c.no_call.resize(R);
        in.read((char*)calls.data(), R * sizeof(pg_call));
        in.read((char*)c.fields.gl_off.data(), (R + 1) * 8);
        in.read((char*)c.fields.gl.data(), n_gl * sizeof(pg_gl));
        in.read((char*)c.kc.data(), R * 2);
        in.read((char*)c.no_call.data(), R);
        if (!in) { std::printf("%s is cut short\n", argv[1]); return 1; }
        c.fields.calls.assign(R, GenotypeCall());
        c.skip.assign(R, 0);
        for (size_t q = 0; q < R; ++q) {
            if ((calls[q].flags & 0xFF) == PG_CALL_OK) { c.fields.calls[q].allele_1 = calls[q].allele_1; c.fields.calls[q].allele_2 = calls[q].allele_2; c.fields.calls[q].quality = calls[q].gq; }
            bool skip = (calls[q].flags & 0xFF) == PG_CALL_DEFERRED || c.fields.gl_off[q + 1] - c.fields.gl_off[q] < 3;
            char buf[32];
            for (uint64_t i = c.fields.gl_off[q]; i < c.fields.gl_off[q + 1] && !skip; ++i) skip = pg_gl_text(c.fields.gl[i], buf, sizeof(buf)) < 0;
            c.skip[q] = skip;
        }
    }
    const int repeats = std::atoi(argv[3]);
    std::printf("{\"chains\": %llu", (unsigned long long)n_chains);
    for (int a = 4; a < argc; ++a) {
        const int T = std::max(1, std::atoi(argv[a]));
        std::vector<double> ms;
        for (int rep = 0; rep <= repeats; ++rep) {   // (the first is the warm-up)
            const auto t0 = std::chrono::steady_clock::now();
            std::atomic<size_t> next(0);
            std::vector<std::thread> pool;
            for (int t = 0; t < T; ++t)
                pool.emplace_back([&] { for (size_t i; (i = next.fetch_add(1)) < chains.size();) form(chains[i]); });
            for (std::thread& t : pool) t.join();
            const double x = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rep) ms.push_back(x);
        }
        std::sort(ms.begin(), ms.end());
        std::printf(", \"threads_%d\": {\"median_ms\": %.3f, \"min_ms\": %.3f, \"max_ms\": %.3f}", T, ms[ms.size() / 2], ms.front(), ms.back());
    }
    uint64_t bytes = 0;
    std::ofstream out(argv[2], std::ios::binary);
    for (const Chain& c : chains) { out.write(c.text.data(), (std::streamsize)c.text.size()); bytes += c.text.size(); }
    std::printf(", \"bytes\": %llu}\n", (unsigned long long)bytes);
    return out ? 0 : 1;
}
