// record_lines_host_join.cpp — the join of a cohort's sample columns into multi-sample VCF lines ON THE HOST, in C++ on T
// threads: what a caller does behind pg_job_fetch_record_text_packed where the device does not join the lines (route (a) of
// tools/bench_record_lines.py, which builds this as a shared library and calls it).  The rule is DESIGN.md 4e-7's: line r of
// contig k = prefix[r], a tab and the text of record r of every sample's chain over k, a newline; nothing if a text is empty.
//
// Chains are sample-major (chain = sample * n_contigs + contig); off[] = every record's first byte in `text`, absolute, chain
// after chain (rec_first[chain] = the chain's first record).  Three passes: the lines' lengths (threads over lines), their
// sum (one thread), the copies (threads over lines).  Returns the bytes written; out_off [n_lines + 1].
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

namespace {

struct Lines {
    uint32_t n_contigs, S;
    const uint64_t* R;           // [n_contigs]
    const uint64_t* line_first;  // [n_contigs + 1]
    const uint64_t* rec_first;   // [S * n_contigs + 1]
    const uint64_t* off;
    const char* text;
    const uint64_t* const* prefix_off;
    const char* const* prefix;
};

template <class F>
void on_threads(int T, uint64_t n, F f) {
    if (T <= 1) { f(0, n); return; }
    std::vector<std::thread> pool;
    for (int t = 0; t < T; ++t) pool.emplace_back([=] { f(n * t / T, n * (t + 1) / T); });
    for (std::thread& t : pool) t.join();
}

// the lines [l0, l1) of all contigs: f(contig, record, global line)
template <class F>
void for_lines(const Lines& L, uint64_t l0, uint64_t l1, F f) {
    uint32_t k = 0;
    for (uint64_t l = l0; l < l1; ++l) {
        while (l >= L.line_first[k + 1]) ++k;
        f(k, l - L.line_first[k], l);
    }
}

}  // namespace

extern "C" uint64_t rl_host_join(uint32_t n_contigs, uint32_t S, const uint64_t* R, const uint64_t* rec_first, const uint64_t* off, const char* text,
                                 const uint64_t* const* prefix_off, const char* const* prefix, uint64_t* out_off, char* out, int threads) {
    std::vector<uint64_t> line_first(n_contigs + 1, 0);
    for (uint32_t k = 0; k < n_contigs; ++k) line_first[k + 1] = line_first[k] + R[k];
    const Lines L = {n_contigs, S, R, line_first.data(), rec_first, off, text, prefix_off, prefix};
    const uint64_t n = line_first.back();
    on_threads(threads, n, [&](uint64_t l0, uint64_t l1) {
        for_lines(L, l0, l1, [&](uint32_t k, uint64_t r, uint64_t l) {
            uint64_t len = L.prefix_off[k][r + 1] - L.prefix_off[k][r] + 1;
            bool host = false;
            for (uint32_t s = 0; s < L.S; ++s) {
                const uint64_t* o = L.off + L.rec_first[(uint64_t)s * L.n_contigs + k] + r;
                host |= o[1] == o[0];
                len += o[1] - o[0] + 1;
            }
            out_off[l + 1] = host ? 0 : len;
        });
    });
    out_off[0] = 0;
    for (uint64_t l = 0; l < n; ++l) out_off[l + 1] += out_off[l];
    on_threads(threads, n, [&](uint64_t l0, uint64_t l1) {
        for_lines(L, l0, l1, [&](uint32_t k, uint64_t r, uint64_t l) {
            if (out_off[l + 1] == out_off[l]) return;
            char* p = out + out_off[l];
            const uint64_t pn = L.prefix_off[k][r + 1] - L.prefix_off[k][r];
            memcpy(p, L.prefix[k] + L.prefix_off[k][r], pn);
            p += pn;
            for (uint32_t s = 0; s < L.S; ++s) {
                const uint64_t* o = L.off + L.rec_first[(uint64_t)s * L.n_contigs + k] + r;
                *p++ = '\t';
                memcpy(p, L.text + o[0], o[1] - o[0]);
                p += o[1] - o[0];
            }
            *p = '\n';
        });
    });
    return out_off[n];
}
