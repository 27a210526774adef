// pg_experiments.h — compile-time knobs of the MEASURING INSTRUMENTS only: ablation masks and in-kernel profilers
// (tools/lean_pipe/exp_pipe.py, exp_timeline.py, tools/exp_viterbi_timeline.py, tools/bench_leanx.py).  A second formulation of
// a step that was measured and not adopted does not live behind a switch: it is in the history and in its record under profiles/.
// The product library defines none of these: every mask is 0 / false and the code it guards folds away.  Builds with a *_EXP mask
// produce WRONG results by design (a part of the step is compiled out so that its share of the time can be read): only their
// timing is of interest (profiles/r03_lean_ablation.txt, r04_lean_chain.txt).  Included by pg_kernels.hip and pg_viterbi.hip.
#pragma once

// general kernel (k_sweep): 1 no column stores, 2 total := 64 C_j, 4 no u round trip, 8 no posterior, 16 no emission
// multiply, 32 / 64 / 128: see the sites.  PG_CHAIN_PROF: cycle counters of a role's launch in DevContig::prof.
#ifndef PG_EXP
#define PG_EXP 0
#endif
static constexpr unsigned kExp = PG_EXP;
#ifdef PG_CHAIN_PROF
static constexpr bool kChainProf = true;
#else
static constexpr bool kChainProf = false;
#endif

// lean step (k_sweep_lean): 1 no column stores, 2 no emission fetches, 4 no MFMA total
#ifndef PG_LEAN_EXP
#define PG_LEAN_EXP 0
#endif
static constexpr unsigned kLeanExp = PG_LEAN_EXP;

// persistent phase 2 (k_sweep_lean<4> + k_post_loop), timing experiments — results WRONG: 1 k_post_loop hands the buffers back
// without forming posteriors, 2 the sweep does not wait for its scratch buffer
#ifndef PG_PERSIST_EXP
#define PG_PERSIST_EXP 0
#endif
static constexpr unsigned kPersistExp = PG_PERSIST_EXP;

// lean-x step (k_sweep_leanx): 1 no column stores, 2 no emission fetches
#ifndef PG_LX_EXP
#define PG_LX_EXP 0
#endif
static constexpr unsigned kLxExp = PG_LX_EXP;   // timing experiments: 1 no column stores, 2 no emission fetches — results WRONG

// -DPG_LEAN_TIMELINE builds only (tools/exp_pipe.py, profiles/r04_lean_chain.txt): s_memtime stamps at the segment
// boundaries of one column step of wave 0, each issued behind a use of the value that ends the segment; the stamps are
// only read behind the step's barrier (reading one earlier would drain the LDS queue with it).  Sums per segment over
// the launches of the sweeps are ADDED to DevContig::prof[32 + segment] (forward role) / [48 + segment] (backward role), [.. + 15] = steps;
// a refill segment (PHASE 5) runs beside them and writes nothing.
#ifdef PG_LEAN_TIMELINE
static constexpr bool kLeanTimeline = true;
#else
static constexpr bool kLeanTimeline = false;
#endif
struct LeanTimeline {
    unsigned long long t[10], acc[10];
    DEVI void init() { if constexpr (kLeanTimeline) { for (int i = 0; i < 10; ++i) { t[i] = 0; acc[i] = 0; } } }
    template <int I>
    DEVI void mark(double dep) {
        if constexpr (kLeanTimeline) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" :: "v"(dep));
            t[I] = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <int N>
    DEVI void fold() {   // behind the barrier: t[0] .. t[N] are this step's stamps
        if constexpr (kLeanTimeline) {
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += t[i + 1] - t[i];
            acc[9] += 1;
        }
    }
    DEVI void write(unsigned long long* o) const {
        if constexpr (kLeanTimeline) { for (int i = 0; i < 9; ++i) o[i] = acc[i]; o[15] = acc[9]; }
    }
    DEVI void add(unsigned long long* o) const {   // (the sweeps of a role are launched one behind the other: their sums add up)
        if constexpr (kLeanTimeline) { for (int i = 0; i < 9; ++i) o[i] += acc[i]; o[15] += acc[9]; }
    }
};

// k_sweep_small16x (pg_small16x.h): 1 no emission reads (e := 1), 2 no parking / no next-record reads (the first record's
// constants and alleles for every column), 4 no record loads, 8 no column stores (phases 1, 3), 16 no row-allele accumulation
// (phase 2), 32 no class sums / bins / aux stores (phase 2), 64 no partner-column loads (phase 2).  (The masks 128 / 256 / 512 named in
// profiles/r05_small16x_ablation*.txt belonged to the per-step record loads those measurements replaced by blocks; they are gone.)
#ifndef PG_X_EXP
#define PG_X_EXP 0
#endif
static constexpr unsigned kXExp = PG_X_EXP;

// -DPG_VIT_TIMELINE builds only (tools/exp_viterbi_timeline.py, profiles/r06_viterbi.txt): s_memtime stamps at the segment
// boundaries of one column step of k_viterbi's wave 0, each issued behind a use of the value that ends the segment; sums per
// segment over the launch go to DevContig::prof[0 .. 11], [15] = steps.  -DPG_VIT_EXP=mask: timing experiments (results WRONG):
// 1 rows: no lo pass, 2 rows: no index pass, 4 column as a whole: no lo pass, 8 no back-pointer stores, 16 no emission fetches.
#ifdef PG_VIT_TIMELINE
static constexpr bool kVitTimeline = true;
#else
static constexpr bool kVitTimeline = false;
#endif
#ifndef PG_VIT_EXP
#define PG_VIT_EXP 0
#endif
static constexpr unsigned kVitExp = PG_VIT_EXP;
struct VitTimeline {
    unsigned long long t[13], acc[13];
    DEVI void init() { if constexpr (kVitTimeline) { for (int i = 0; i < 13; ++i) { t[i] = 0; acc[i] = 0; } } }
    template <int I>
    DEVI void mark(double dep) {
        if constexpr (kVitTimeline) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" :: "v"(dep));
            t[I] = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <int I>
    DEVI void mark_u(unsigned dep) {
        if constexpr (kVitTimeline) {
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" :: "v"(dep));
            t[I] = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <int N>
    DEVI void fold() {
        if constexpr (kVitTimeline) {
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += t[i + 1] - t[i];
            acc[12] += 1;
        }
    }
    DEVI void write(unsigned long long* o) const {
        if constexpr (kVitTimeline) { for (int i = 0; i < 12; ++i) o[i] = acc[i]; o[15] = acc[12]; }
    }
};
