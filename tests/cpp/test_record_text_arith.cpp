// test_record_text_arith.cpp — pgx_record_text / pgx_record_text_len / pgx_record_text_bound (pangenie_amd/csrc/pg_calls.h), the
// bytes of the VCF sample column GT:GQ:GL:KC, against a restatement of what the host prints of the same fields through an
// ostringstream (device_field, pangenie_amd/host/graph_io.cpp).  Stand-alone: g++ -I pangenie_amd/csrc, no device, no library.
//
// The value sets are those of tests/test_record_text_values_gpu.py: every exponent -99 .. 99 x both signs x the mantissas
// {1000, 1200, 1230, 1234, 1204, 9000, 9999, 5050}; every mantissa 1000 .. 9999 x both signs at exp10 in {-5, -4, -1, 0, 3, 4};
// -inf; 0.  Records of three values each, under every call flag, with and without no_call, with every KC width.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "pg_calls.h"

static long n_checked = 0, n_failed = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        ++n_checked;                                              \
        if (!(cond)) {                                            \
            if (++n_failed <= 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

static pg_call call_of(unsigned a1, unsigned a2, unsigned gq, unsigned flags) {
    pg_call c;
    c.allele_1 = (uint16_t)a1; c.allele_2 = (uint16_t)a2; c.gq = (uint16_t)gq; c.flags = (uint16_t)flags;
    return c;
}

// What the host's stream prints; `hosts` = the record is one the host completes from bins (it cannot be printed from these fields).
static std::string host_text(pg_call c, const std::vector<pg_gl>& gl, unsigned short kc, bool no_call, bool* hosts) {
    *hosts = (c.flags & 0xFF) == PGX_CALL_DEFERRED || gl.size() < 3;
    std::ostringstream out;
    const bool ok = (c.flags & 0xFF) == PGX_CALL_OK;   // (the host's GenotypeCall has alleles >= 0 exactly then)
    if (!no_call && ok) out << (int)c.allele_1 << "/" << (int)c.allele_2 << ":" << (int)c.gq << ":";
    else out << ".:.:";
    for (size_t j = 0; j < gl.size(); ++j) {
        char text[32];
        if (pgx_gl_text(gl[j], text, sizeof(text)) < 0) { *hosts = true; return ""; }
        out << (j ? "," : "") << text;
    }
    out << ":" << kc;
    return out.str();
}

static void check_record(pg_call c, const std::vector<pg_gl>& gl, unsigned short kc, bool no_call) {
    bool hosts = false;
    const std::string want = host_text(c, gl, kc, no_call, &hosts);
    const uint64_t bound = pgx_record_text_bound(1, gl.size());
    std::vector<char> buf(bound + 8, '#');
    const uint32_t len = pgx_record_text_len(c, gl.data(), (uint32_t)gl.size(), kc, no_call);
    const uint32_t put = pgx_record_text(c, gl.data(), (uint32_t)gl.size(), kc, no_call, buf.data());
    CHECK(len == put, "length %u, written %u", len, put);
    if (hosts) {
        CHECK(len == 0, "a record of the host's has length %u", len);
        CHECK(buf[0] == '#', "a record of the host's was written");
        return;
    }
    CHECK(put <= bound, "%u bytes, bound %llu", put, (unsigned long long)bound);
    CHECK(put == want.size() && memcmp(buf.data(), want.data(), want.size()) == 0, "got '%.*s' want '%s'", (int)put, buf.data(), want.c_str());
    CHECK(buf[put] == '#', "wrote behind the text");
}

int main() {
    std::vector<pg_gl> values;
    const int mants[8] = {1000, 1200, 1230, 1234, 1204, 9000, 9999, 5050};
    for (int x = -99; x <= 99; ++x)
        for (int sgn = -1; sgn <= 1; sgn += 2)
            for (int m : mants) values.push_back(pgx_gl_of(sgn * m, x));
    const int exps[6] = {-5, -4, -1, 0, 3, 4};
    for (int x : exps)
        for (int sgn = -1; sgn <= 1; sgn += 2)
            for (int m = 1000; m <= 9999; ++m) values.push_back(pgx_gl_of(sgn * m, x));
    values.push_back(pgx_gl_neg_inf());
    values.push_back(pgx_gl_of(0, 0));
    while (values.size() % 3) values.push_back(pgx_gl_neg_inf());

    const pg_call calls[7] = {call_of(0, 1, 37, PGX_CALL_OK), call_of(255, 255, 10000, PGX_CALL_OK), call_of(0, 0, 10000, PGX_CALL_OK | PGX_CALL_EMPTY),
                              call_of(0xFFFF, 0xFFFF, 0, PGX_CALL_NONE), call_of(0xFFFF, 0xFFFF, 0, PGX_CALL_NOT_UNIQUE),
                              call_of(0xFFFF, 0xFFFF, 0, PGX_CALL_DEFERRED), call_of(12, 107, 192, PGX_CALL_OK)};
    const unsigned short kcs[6] = {0, 7, 42, 999, 1000, 65535};
    // every value, three to a record, the calls, KC widths and no_call taking turns
    for (size_t i = 0, k = 0; i < values.size(); i += 3, ++k) {
        const std::vector<pg_gl> gl(values.begin() + i, values.begin() + i + 3);
        check_record(calls[k % 7], gl, kcs[k % 6], (k / 7) % 2 != 0);
        check_record(calls[0], gl, 17, false);
    }
    // every call x no_call x KC on one set of values, with 1, 2, 3, 6 and 10 of them
    for (const pg_call& c : calls)
        for (int nc = 0; nc < 2; ++nc)
            for (unsigned short kc : kcs)
                for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)6, (size_t)10})
                    check_record(c, std::vector<pg_gl>(values.begin() + 40, values.begin() + 40 + n), kc, nc != 0);
    // a deferred value and encodings that are no value, first, in the middle and last: the host's
    const pg_gl bad[6] = {pgx_gl_deferred(), pgx_gl_of(0, 5), pgx_gl_of(999, 0), pgx_gl_of(10000, 0), pgx_gl_of(1234, 100), pgx_gl_of(-1234, -100)};
    for (const pg_gl& b : bad)
        for (size_t at = 0; at < 3; ++at) {
            std::vector<pg_gl> gl(values.begin(), values.begin() + 3);
            gl[at] = b;
            bool hosts = false;
            (void)host_text(calls[0], gl, 5, false, &hosts);
            CHECK(hosts, "the restatement prints a value that is none");
            check_record(calls[0], gl, 5, false);
        }
    // the bound is reached: 255/255:10000: + n times -1.234e-05 + :65535
    for (size_t n : {(size_t)3, (size_t)6, (size_t)21, (size_t)820, (size_t)32896}) {
        const std::vector<pg_gl> gl(n, pgx_gl_of(-1234, -5));
        check_record(calls[1], gl, 65535, false);
        const uint32_t len = pgx_record_text_len(calls[1], gl.data(), (uint32_t)n, 65535, false);
        CHECK(len == pgx_record_text_bound(1, n), "%u bytes, bound %llu", len, (unsigned long long)pgx_record_text_bound(1, n));
        const std::vector<pg_gl> gl2(n, pgx_gl_of(-1234, -4));   // -0.0001234: ten bytes too
        CHECK(pgx_record_text_len(calls[1], gl2.data(), (uint32_t)n, 65535, false) == pgx_record_text_bound(1, n), "fixed notation misses the bound");
    }
    CHECK(pgx_record_text_bound(7, 100) == 19u * 7 + 11u * 100, "bound");
    printf("%ld checks, %ld failed\n", n_checked, n_failed);
    return n_failed ? 1 : 0;
}
