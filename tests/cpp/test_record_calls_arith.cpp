// test_record_calls_arith.cpp — pgx_decide_record (pangenie_amd/csrc/pg_calls.h), the call of one VCF record from its
// bubble's bins, against a long double restatement of what the host does (DESIGN.md 4e "Records"): normalise the
// bubble, fold it onto the record's alleles in a std::map with +=, drop the genotypes over undefined alleles and
// renormalise, likeliest genotype with >= and the 1e-10 tie rule, quality from log10l.  Bit for bit: GT, GQ and flag.
// Stand-alone: g++ -std=c++17 -I pangenie_amd/csrc, no device.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <map>
#include <utility>
#include <vector>

#include "pg_calls.h"

static_assert(LDBL_MANT_DIG == 64, "this test needs the x87 80-bit long double");

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<uint64_t> g_tm(PG_GQ_STEPS);
static std::vector<int32_t> g_te(PG_GQ_STEPS);

struct Bubble {
    bool kept = true;
    std::vector<uint16_t> id;     // [A] allele id of every slot
    std::vector<uint8_t> pres;    // [A]
    std::vector<double> m;        // [A (A + 1) / 2] bins, slot pairs a <= b in row order
    std::vector<int32_t> e;
};
struct Record {
    std::vector<uint16_t> own;    // by bubble allele ID: the record allele it carries
    std::vector<uint16_t> vcf;    // [n_alleles] index among the defined alleles, 0xFFFF: undefined
    bool has_undefined() const { for (uint16_t x : vcf) if (x == 0xFFFF) return true; return false; }
};
struct Call { uint32_t flags, a1, a2, gq; };

// ---- the host route in long double ----
static Call call_ld(const Bubble& b, const Record& r) {
    typedef std::pair<unsigned, unsigned> G;
    const size_t A = b.id.size();
    std::vector<std::pair<G, long double>> N;   // the bubble's map: keys in bin order
    size_t bin = 0;
    for (size_t x = 0; x < A; ++x)
        for (size_t y = x; y < A; ++y, ++bin)
            if (b.kept && b.pres[x] && b.pres[y]) N.push_back({G(b.id[x], b.id[y]), ldexpl((long double)b.m[bin], b.e[bin])});
    long double sum = 0.0L;
    for (auto& kv : N) sum += kv.second;
    if (sum > 0) for (auto& kv : N) kv.second = kv.second / sum;
    std::map<G, long double> F;                  // Variant::separate_variants
    for (auto& kv : N) {
        unsigned ra = r.own[kv.first.first], rb = r.own[kv.first.second];
        if (ra > rb) std::swap(ra, rb);
        F[G(ra, rb)] += kv.second;
    }
    if (F.empty()) F[G(0, 0)] = 1.0L;
    if (r.has_undefined()) {                     // get_specific_likelihoods over the defined alleles
        std::map<G, long double> S;
        long double sum2 = 0.0L;
        for (auto& kv : F) {
            if (r.vcf[kv.first.first] == 0xFFFF || r.vcf[kv.first.second] == 0xFFFF) continue;
            S[G(r.vcf[kv.first.first], r.vcf[kv.first.second])] += kv.second;
            sum2 += kv.second;
        }
        if (sum2 > 0) for (auto& kv : S) kv.second = kv.second / sum2;
        F.swap(S);
    }
    Call c = {PGX_CALL_NONE, 0xFFFF, 0xFFFF, 0};
    if (F.empty()) return c;
    long double best = 0.0L;                     // get_likeliest_genotype
    G bg(0, 0);
    for (auto& kv : F) if (kv.second >= best) { best = kv.second; bg = kv.first; }
    bool unique = true;
    for (auto& kv : F) if (kv.first != bg && fabsl(kv.second - best) < 0.0000000001) unique = false;
    if (!(best > 0.0L)) return c;
    if (!unique) { c.flags = PGX_CALL_NOT_UNIQUE; return c; }
    c.flags = PGX_CALL_OK;
    c.a1 = bg.first; c.a2 = bg.second;
    const long double pw = 1.0L - best;          // get_genotype_quality
    c.gq = pw > 0.0 ? (uint32_t)(size_t)(-10 * log10l(pw)) : 10000u;
    return c;
}

// ---- the same through pgx_decide_record ----
struct BubbleKeys {
    const Bubble* b;
    const Record* r;
    size_t x, y, bin;
    void start() { x = 0; y = 0; bin = 0; }
    bool next(pgx* v, uint32_t* key) {
        const size_t A = b->id.size();
        while (x < A) {
            const size_t cx = x, cy = y, cbin = bin;
            ++bin;
            if (++y == A) { ++x; y = x; }
            if (b->kept && b->pres[cx] && b->pres[cy]) {
                uint32_t ra = r->own[b->id[cx]], rb = r->own[b->id[cy]];
                if (ra > rb) std::swap(ra, rb);
                *v = pgx_from_bin(b->m[cbin], b->e[cbin]);
                *key = (ra << 16) | rb;
                return true;
            }
        }
        return false;
    }
};
struct DefinedOf {
    const Record* r;
    bool operator()(uint32_t a) const { return r->vcf[a] != 0xFFFF; }
};

static Call call_pgx(const Bubble& b, const Record& r) {
    BubbleKeys keys = {&b, &r, 0, 0, 0};
    DefinedOf def = {&r};
    const pgx_record_decision d = pgx_decide_record(keys, r.has_undefined(), def, g_tm.data(), g_te.data());
    Call c = {d.flags, 0xFFFF, 0xFFFF, 0};
    if ((d.flags & 0xFFu) == PGX_CALL_OK) { c.a1 = r.vcf[d.key >> 16]; c.a2 = r.vcf[d.key & 0xFFFFu]; c.gq = d.gq; }
    return c;
}

static void check(const Bubble& b, const Record& r, const char* what) {
    const Call want = call_ld(b, r), got = call_pgx(b, r);
    CHECK((got.flags & 0xFFu) == want.flags && got.a1 == want.a1 && got.a2 == want.a2 && got.gq == want.gq,
          "%s: A %zu: flags %u GT %u/%u GQ %u, long double: flags %u GT %u/%u GQ %u", what, b.id.size(), got.flags, got.a1, got.a2, got.gq,
          want.flags, want.a1, want.a2, want.gq);
}

static double rnd_mant() { return ldexp((double)((rnd() >> 11) | (1ull << 52)), -53); }

static Record rnd_record(unsigned n_ids) {
    Record r;
    const unsigned nA = 1 + rnd() % (n_ids < 6 ? n_ids + 1 : 6);
    r.own.resize(n_ids);
    for (unsigned i = 0; i < n_ids; ++i) r.own[i] = (uint16_t)(i == 0 ? 0 : rnd() % nA);
    r.vcf.resize(nA);
    uint16_t d = 0;
    const bool undef = rnd() % 3 == 0;
    for (unsigned a = 0; a < nA; ++a) r.vcf[a] = (a == 0 || !undef || rnd() % 3) ? d++ : (uint16_t)0xFFFF;
    return r;
}

static void test_random() {
    for (int it = 0; it < 220000; ++it) {
        Bubble b;
        const unsigned A = 2 + rnd() % 11, spread = (rnd() % 4 == 0) ? 401 : (rnd() % 2 ? 8 : 70);
        uint16_t id = 0;
        for (unsigned a = 0; a < A; ++a) { b.id.push_back(id); id += 1 + (rnd() % 5 == 0); b.pres.push_back(rnd() % 6 != 0); }
        b.kept = rnd() % 40 != 0;
        const int32_t base = -(int32_t)(rnd() % 9000);
        for (unsigned k = 0; k < A * (A + 1) / 2; ++k) {
            b.m.push_back(rnd() % 13 == 0 ? 0.0 : rnd_mant());
            b.e.push_back(base - (int32_t)(rnd() % spread));
        }
        if (rnd() % 8 == 0) { const size_t j = rnd() % b.m.size(), k = rnd() % b.m.size(); b.m[k] = b.m[j]; b.e[k] = b.e[j]; }
        const unsigned n_rec = 1 + rnd() % 4;
        for (unsigned q = 0; q < n_rec; ++q) check(b, rnd_record(id), "random");
    }
}

// ---- constructed cases: every sum is exactly 1, so that a quotient is its bin ----
static Bubble bubble(std::vector<uint16_t> id, std::vector<uint8_t> pres, std::vector<double> m, std::vector<int32_t> e) {
    Bubble b;
    b.id = id; b.pres = pres; b.m = m; b.e = e;
    return b;
}
static Record record(std::vector<uint16_t> own, std::vector<uint16_t> vcf) {
    Record r;
    r.own = own; r.vcf = vcf;
    return r;
}
static const double U = 0x1p-64;   // one unit in the last place of a long double in [1/2, 1)

static void expect(const Bubble& b, const Record& r, uint32_t flags, uint32_t a1, uint32_t a2, uint32_t gq, const char* what) {
    check(b, r, what);
    const Call got = call_pgx(b, r);
    CHECK(got.flags == flags && got.a1 == a1 && got.a2 == a2 && got.gq == gq, "%s: flags %#x GT %u/%u GQ %u, expected %#x %u/%u %u", what, got.flags,
          got.a1, got.a2, got.gq, flags, a1, a2, gq);
}

static void test_constructed() {
    const std::vector<int32_t> z6(6, 0);
    const std::vector<uint16_t> ids3 = {0, 1, 2};
    const std::vector<uint8_t> p3 = {1, 1, 1};
    // empty maps
    Bubble nk = bubble(ids3, p3, {0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6);
    nk.kept = false;
    expect(nk, record({0, 1, 0}, {0, 1}), PGX_CALL_OK | PGX_CALL_EMPTY, 0, 0, 10000, "not kept");
    expect(bubble(ids3, {0, 0, 0}, {0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6), record({0, 1, 1}, {0, 0xFFFF}), PGX_CALL_OK | PGX_CALL_EMPTY, 0, 0,
           10000, "no allele present");
    expect(bubble(ids3, p3, {0, 0, 0, 0, 0, 0}, z6), record({0, 1, 0}, {0, 1}), PGX_CALL_NONE, 0xFFFF, 0xFFFF, 0, "all zero");
    // the fold creates a tie: F(0,0) = 1/4 + 3/16 + 1/16, F(0,1) = 3/8 + 1/8
    expect(bubble(ids3, p3, {0.25, 0.375, 0.1875, 0, 0.125, 0.0625}, z6), record({0, 1, 0}, {0, 1}), PGX_CALL_NOT_UNIQUE, 0xFFFF, 0xFFFF, 0,
           "fold creates a tie");
    // ... resolves one: (1,1) and (1,2) tie in the bubble, both are 1/1 of the record
    expect(bubble(ids3, p3, {0.25, 0, 0, 0.375, 0.375, 0}, z6), record({0, 1, 1}, {0, 1}), PGX_CALL_OK, 1, 1, 6, "fold resolves a tie");
    // the likeliest folded genotype holds the undefined allele 1: the call moves to 2/2, GT 1/1, 1/4 of 1/2
    expect(bubble(ids3, p3, {0.125, 0.5, 0.125, 0, 0, 0.25}, z6), record({0, 1, 2}, {0, 0xFFFF, 1}), PGX_CALL_OK, 1, 1, 3, "likeliest is undefined");
    expect(bubble(ids3, p3, {0, 0.5, 0, 0.5, 0, 0}, z6), record({0, 1, 2}, {0, 0xFFFF, 1}), PGX_CALL_NONE, 0xFFFF, 0xFFFF, 0, "defined keys all zero");
    // best = 1 - m 2^-64 only as the sum of two bins
    const uint32_t gqs[5] = {10000, 192, 189, 187, 186};
    for (int m = 0; m <= 4; ++m)
        expect(bubble(ids3, p3, {1.0 - 0x1p-53, (2048.0 - m) * U, 0, 0, 0, m * U}, z6), record({0, 0, 1}, {0, 1}), PGX_CALL_OK, 0, 0, gqs[m], "1 - m 2^-64");
    // three quotients onto one key: (q1 + q2) + q3 = 1 - 2u (a tie to even, then a sticky quarter), (q2 + q3) + q1 = 1 - u
    const double q1 = 1.0 - 0x1p-53, q2 = 2046.5 * U, q3 = 0.25 * U;
    expect(bubble(ids3, p3, {q1, q2, 0, q3, 0, 2 * U}, z6), record({0, 0, 1}, {0, 1}), PGX_CALL_OK, 0, 0, 189, "addition order q1 q2 q3");
    expect(bubble(ids3, p3, {q2, q3, 0, q1, 0, 2 * U}, z6), record({0, 0, 1}, {0, 1}), PGX_CALL_OK, 0, 0, 192, "addition order q2 q3 q1");
    // a runner-up next to the tie threshold after the fold
    for (int s = -1; s <= 1; s += 2) {
        const double t = 1e-10 * (1.0 + s * 0x1p-20);
        expect(bubble(ids3, p3, {0.25 * (1.0 + t), 0, 0.25 * (1.0 + t), 0.5 * (1.0 - t), 0, 0}, z6), record({0, 1, 0}, {0, 1}),
               s < 0 ? PGX_CALL_NOT_UNIQUE : PGX_CALL_OK, s < 0 ? 0xFFFF : 0, s < 0 ? 0xFFFF : 0, s < 0 ? 0 : 3, "runner-up at the threshold");
    }
    // allele ids that are not slots, an absent allele in the middle
    expect(bubble({0, 2, 5, 7}, {1, 0, 1, 1}, {0.125, 9, 0.125, 0, 9, 9, 9, 0.25, 0.5, 0}, std::vector<int32_t>(10, 0)),
           record({0, 9, 1, 9, 9, 1, 9, 2}, {0, 1, 0xFFFF}), PGX_CALL_OK, 1, 1, 3, "ids are not slots");
    // both sides of 2^-16300
    Bubble lo = bubble(ids3, p3, {0.5, 0.75, 0.5, 0.5, 0.5, 0.5}, {-16310, -16301, -16400, -16330, -16305, -16302});
    CHECK(call_pgx(lo, record({0, 1, 0}, {0, 1})).flags == PGX_CALL_DEFERRED && call_pgx(lo, record({0, 1, 1}, {0, 0xFFFF})).flags == PGX_CALL_DEFERRED,
          "largest bin below 2^-16300: every record is deferred");
    lo.e[1] = -16299;
    check(lo, record({0, 1, 0}, {0, 1}), "next to the deferral cut");
    CHECK(call_pgx(lo, record({0, 1, 0}, {0, 1})).flags != PGX_CALL_DEFERRED, "largest bin at 2^-16300 is decided");
}

int main() {
    if (pgx_build_gq_table(g_tm.data(), g_te.data()) != 0) { printf("the GQ table could not be built\n"); return 2; }
    test_random();
    test_constructed();
    printf("%ld checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
