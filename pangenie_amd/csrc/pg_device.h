// pg_device.h — device-side data layout shared by the HIP kernels and the C-ABI shim.
//
// HBM layout per contig (one chain = one (contig, path-subset)):
//   inputs        : the SoA of include/pangenie_hmm.h, uploaded verbatim
//   vrec[V][RB]   : per-variant record written by k_prep (emission table, local allele
//                   index of every selected path, emission exponent)
//   colrec[C][RB] : the same records gathered in column order by k_records, with the
//                   Li-Stephens constants of the gap (c-1 -> c) filled in.  This is the
//                   ONE stream the chain kernels read besides the forward columns.
//   fwd[C][HP*HP] : column slots (fp64): slot c holds the forward column of c < C/2 and the
//                   backward column of c >= C/2 — written once in sweep phase 1, read once in
//                   sweep phase 2: the 16*H^2 algorithmic bytes per column.
//   part[C][part_slots/2][T][2] : (fused mode) per-thread posterior partials by row-allele pair,
//                   reduced by k_bins
//   scratch / handoff-free chunk buffers : (chunked mode) see DevContig::scratch
//   vpair[V][..]  : (mantissa, exponent) of the emission product of every local allele pair of a
//                   variant — applied ONCE to a finished posterior bin (k_bins / k_post), so a bin keeps
//                   full relative precision however small its emission is
//   wide[..]      : emission tables of columns with more than PG_AMAX alleles on the selected paths
//   xbuf[2][HP*HP]: generic sweep kernel only (HP >= 256): the column after the emission multiply
//   lik / lik_exp : outputs, one (mantissa, exponent) pair per genotype bin
//   vit_*         : (run_phasing) Viterbi backtrace and haplotypes, see DevContig
#pragma once
#include <stddef.h>
#include <stdint.h>

#define PG_AMAX 5                 // max distinct alleles on the selected paths of a NARROW column (table inside the record)
#define PG_ESTRIDE (PG_AMAX + 1)  // row stride of the expanded emission table; row/col PG_AMAX = 0 (phantom paths)
#define PG_ETAB (PG_ESTRIDE * PG_ESTRIDE)
#define PG_MAX_ALLELES_PER_VARIANT 256  // all alleles of one UniqueKmers object (k_prep keeps their presence in a 256-bit LDS bitmap)
#define PG_MAX_PATHS 1024               // selected paths per chain (HP = 16..128: register-resident kernels; 256..1024: generic kernel)
#define PG_PHANTOM 255

// byte offsets inside a record
#define PG_REC_C0 0
#define PG_REC_C1 8
#define PG_REC_C2 16
#define PG_REC_KAPPA 24
#define PG_REC_VARIANT 32
#define PG_REC_EXP 36
#define PG_REC_NLOCAL 40
#define PG_REC_FLAGS 41
#define PG_REC_LOCAL_SLOT 48  // u16[8] (PG_AMAX used)
#define PG_REC_BITS1 64       // u64[2]: bit p = selected path p carries local allele 1 (biallelic fast path)
#define PG_REC_E 80           // double[PG_ETAB]
#define PG_REC_ALLELES (80 + 8 * PG_ETAB)  // u8[HP]
#define PG_REC_FLAG_ALLZERO 1
#define PG_REC_FLAG_WIDE 2    // more than PG_AMAX alleles on the selected paths: table in DevContig::wide
#define PG_REC_WIDE_IDX 44    // u32: byte offset / 16 of the variant's wide entry inside DevContig::wide
#define PG_REC_AUX 60         // u32: byte offset / 16 of the variant's slot inside DevContig::aux (PG_WIDE_NONE: none); the last two of the eight local-slot entries
// INVARIANT of vrec: the records of a job are zeroed ONCE, when the job is built (pg_shim.cpp), and k_prep_bi stores only
// the 16-byte pieces of a biallelic object's record that are not zero by construction (header, row bits, four table entries,
// path alleles).  That is sound because the kernel that prepares an object is a function of the index shape alone (alleles and
// k-mers per variant, which pg_job_upload holds fixed) and no kernel writes anything else into a record: a new writer into
// vrec has to keep both, or store whole records.  The split path (below) has no vrec at all.

// Wide entries (columns with PG_AMAX < n_local <= PG_WIDE_MAX distinct alleles on the selected paths;
// chunked sweep mode — or, round 5, a fused job's 16-path chain on k_sweep_small16x): the emission table no longer fits the column record, so it lives in a
// side buffer.  With S = n_local + 1 (row/column n_local is zero: phantom paths) an entry holds
//   double  E [S][S]   emission products scaled by 2^-X (symmetric), read by the recursion
//   double  Pm[S][S]   mantissa in [0.5,1) (or 0) of the unscaled product of the local pair
//   int32   Pe[S][S]   its exponent                      (Pm, Pe: applied to finished bins)
//   u16     slot[n_local]  local allele -> allele slot of the variant
// The host reserves room for S = min(A, H) + 1 per variant with more than PG_AMAX alleles.
#define PG_WIDE_MAX 254
#define PG_WIDE_NONE 0xFFFFFFFFu
static inline uint64_t pg_wide_entry_bytes(uint32_t n_local) {
    const uint64_t s = (uint64_t)n_local + 1;
    return (s * s * 20 + (uint64_t)n_local * 2 + 15) & ~(uint64_t)15;
}
#define PG_WIDE_OFF_PM(S) ((size_t)(S) * (S) * 8)
#define PG_WIDE_OFF_PE(S) ((size_t)(S) * (S) * 16)
#define PG_WIDE_OFF_SLOT(S) ((size_t)(S) * (S) * 20)

// Chunked mode: the store-only chunk sweeps of phase 2 write into PG_SCRATCH_BUFS rotating scratch buffers (two roles each),
// k_post reads a finished one from a second stream.  Three (round 5; two before): with two, sweep i + 2 had to wait for the
// posteriors of chunk i, and while all chains of a genome are still running k_post takes longer than a sweep (3.0 against
// 2.7 ms on genome24_h64) — 6 ms of idle gaps between the 50 chunk sweeps (profiles/r05_genome24_timeline.txt); with three the
// early deficit is worked off once the short chains have ended.
#ifndef PG_SCRATCH_BUFS
#define PG_SCRATCH_BUFS 3u
#endif
#define PG_SCR_BUF(c) ((c) % PG_SCRATCH_BUFS)
#define PG_SYNC_NEXT 16u
#define PG_SYNC_DONE 17u
#define PG_SYNC_READY 32u   // chunks with both roles stored, republished by k_post_loop's watcher wave (what its other waves poll)
#define PG_SYNC_WORDS 48u   // DevContig::sync: three 64-byte lines per chain

// Column biases: stored forward columns (before the emission multiply) sum to about
// 2^PG_BIAS_F, stored backward columns to about 2^PG_BIAS_B times their emission-weighted mass.
#define PG_BIAS_F 400
#define PG_BIAS_B 400

// (mantissa, exponent) pair tables of narrow variants: vpair[v] = double m[NP] then int32 e[NP],
// NP = pair_n (pair_n + 1) / 2 padded to even, index la * pair_n - la (la - 1) / 2 + (lb - la)
static inline uint32_t pg_pair_count(uint32_t pair_n) { return ((pair_n * (pair_n + 1) / 2) + 1u) & ~1u; }
static inline uint32_t pg_pair_bytes(uint32_t pair_n) { return pg_pair_count(pair_n) * 12u; }

static inline uint32_t pg_rec_bytes(uint32_t hp) { return (PG_REC_ALLELES + hp + 63u) & ~63u; }

// error bits raised by kernels in DevContig::err
#define PG_DEVERR_ALLELE_NOT_FOUND 1u
#define PG_DEVERR_TOO_MANY_ALLELES 2u
#define PG_DEVERR_TOO_MANY_LOCAL 4u
#define PG_DEVERR_SYNC_TIMEOUT 16u // a persistent phase-2 kernel (k_sweep_lean<4> / k_post_loop) gave up waiting for its partner's chunk flag
#define PG_DEVERR_WIDE_FUSED 8u   // a wide column reached a fused bins kernel that has no path for it (a single-column chain of k_sweep_small16x's job)

struct DevTable {
    uint32_t cov_min, cov_max, count_max;  // dense box [cov_min,cov_max) x [0,count_max)
    uint32_t pad;
    double reg;           // regularization constant (on-the-fly path)
    const double* mant;   // [cov-cov_min][count][3]
    const int32_t* expo;  // [cov-cov_min][count][3]
    // the same entries as ONE 32-byte piece each, {m0, m1, m2, int16 e0, e1, e2, 0}: two 16-byte loads per k-mer where the
    // split arrays take six (the sample-level kernels of the split path, pg_split.h; every exponent of the table lies in
    // [PG_LD_MIN_EXP, 1], so int16 holds it)
    const unsigned char* packed;   // [cov-cov_min][count][32]
};

// ------------------------------------------------------------------------------------------------------------------
//  The split path (round 6): what depends on the INDEX alone is formed once, when the index is uploaded, and shared by
//  every chain (sample) over that index contig; a run of the job forms only what depends on the sample's read counts.
//  reference: the index is sample-independent, update_readcount / set_coverage are the per-sample part
//  (src/commands.cpp:118-138); the column list hangs on path alleles and undefined flags (src/columnindexer.cpp:8-33), the
//  transition probabilities on positions (src/transitionprobabilitycomputer.cpp:8-19), the emissions on the counts
//  (src/emissionprobabilitycomputer.cpp:9-53).
//
//  For EVERY chain (all kernels): kept[V], allele_present[sumA], col_variant[C], n_cols, col_of[V] are per index contig
//  (k_index_scan + k_compact at upload; no k_compact in a run).
//  For the 16-path chains of fused jobs (DevContig::split; k_sweep_small16 / k_sweep_small16x both phases), per COLUMN:
//    ix_pd [C][32]  what the sample-level emission kernel needs of a column: {variant, first k-mer, K | flags << 8,
//                   k-mer bits of allele slot 0, of slot 1 (biallelic objects), 0, 0, 0}
//    ix_rec[C][64]  what the sweeps need besides the emissions.  split == 1 (every object biallelic): {c0, c1, c2, kappa,
//                   row bits, 0, 0, 0} — copied into the 64-byte record of k_sweep_small16 by the emission kernel;
//                   split == 2: bytes 128 .. 191 of k_sweep_small16x's record (header, constants, row offsets), read
//                   by the sweep as a second stream
//    ix_bin[C][32]  what the bins kernels need: {first bin of the variant, variant, aux slot, A (u16), nlocal, flags,
//                   allele slot of local allele 0 .. 4 (u16), paths carrying local allele 0 .. 4 (u8), 0}
//  and per chain, in COLUMN order, written by the emission kernels k_prep_s_* every run:
//    split == 1: frec[C][64]  {c0, c1, c2, kappa, E'00, E'01, E'11, row bits | flags << 16 | X << 32}
//    split == 2: frec[C][128] the fifteen table entries (tri_local order; a wide column: its sixteen raw local alleles in
//                the first sixteen bytes) then {int32 X, uint32 flags}
//    cprec[C][192] only for columns flagged PG_SREC_FLAG_PRECISE: the unscaled products as (mantissa[16], exponent[16]).
//  The bins kernels recover a pair's (mantissa, exponent) from the scaled entry and X — E' = m 2^(e - X) exactly unless
//  that is subnormal: a column with such an entry (a present pair 2^-1021 below the column's largest) is flagged and its
//  products go to cprec as well.  No vrec / colrec / vpair for such chains.
#define PG_IXPD_BYTES 32u
#define PG_IXREC_BYTES 64u
#define PG_IXBIN_BYTES 32u
#define PG_SREC1_BYTES 64u
#define PG_SREC2_BYTES 128u
#define PG_CPREC_BYTES 192u
#define PG_COL_NONE 0xFFFFFFFFu
#define PG_IXPD_U0 0x100u        // kf: K | these
#define PG_IXPD_U1 0x200u
#define PG_IXPD_HAS0 0x400u
#define PG_IXPD_HAS1 0x800u
#define PG_SREC_FLAG_ALLZERO 1u  // (= PG_REC_FLAG_ALLZERO)
#define PG_SREC_FLAG_WIDE 2u     // (= PG_REC_FLAG_WIDE)
#define PG_SREC_FLAG_PRECISE 4u
struct IxBin {
    uint32_t g0, v, aux;
    uint16_t A;
    uint8_t nl, flags;
    uint16_t ls[5];
    uint8_t cnt[5];
    uint8_t pad;
};

struct DevContig {
    uint32_t V, H, HP, RB;
    uint32_t T;            // entries of posterior partials per column and slot pair: threads per chain workgroup = HP*HP/R (half of them at HP = 32)
    uint32_t pad0;
    double dist_scale;     // 0.000004 * recombrate * effective_N
    int32_t uniform;
    uint32_t debug;        // bit 3: in-kernel cycle counters (-DPG_CHAIN_PROF builds only; no effect in the product build)
    uint32_t part_slots;   // allele slots per column in `part` = min(PG_AMAX, max alleles of a variant)
    uint32_t pair_n;       // local alleles the vpair tables are laid out for = min(PG_AMAX, max alleles of a variant)
    // inputs
    const uint64_t* pos;
    const uint16_t* cov;
    const uint32_t* kmer_off;
    const uint16_t* kmer_count;
    const uint32_t* allele_off;
    const uint16_t* allele_id;
    const uint8_t*  allele_flags;
    const uint16_t* allele_koff;
    const uint32_t* allele_kmask;
    const uint16_t* path_allele;
    const uint64_t* geno_off;
    // intermediates
    uint8_t*  vrec;
    uint8_t*  kept;
    uint8_t*  allele_present;
    uint32_t* n_cols;
    uint32_t* col_variant;
    uint8_t*  colrec;
    double*   fwd;
    double*   part;
    double*   fscale;        // [V] mantissa m of the scale applied to forward column c (see chain kernels)
    double*   bscale;        // [V] same for the backward column
    double*   bsum;          // [V] sum of the stored backward column (hand-over between the phases)
    uint8_t*  fwd_fallback;  // [V] column c fell back to the uniform forward column (fsum := 1, no emission scale)
    // chunked mode (few chains, see pg_shim.cpp): phase 2 is run in chunks of chunk_cols columns per
    // half-chain that only STORE their columns into this scratch ([PG_SCRATCH_BUFS buffers][2 roles][chunk_cols][HP*HP],
    // forward role first); k_post forms the posteriors of a finished chunk on the idle CUs.
    double*   scratch;
    // persistent chunked phase 2 (all chains lean, few of them — pg_shim.cpp `persist`): ONE launch of k_sweep_lean<4> walks
    // every chunk of a half-chain and ONE launch of k_post_loop every chunk's posteriors; the two hand chunks over through
    // these words (zeroed at the start of every run; agent-scope release / acquire):
    //   sync[0] / sync[1]      = chunks the forward / backward role has finished storing (written by the sweep; a 64-byte line of their own),
    //   sync[PG_SYNC_NEXT]     = the next column slot to hand out (k_post_loop's work queue: chunk after chunk, 2 chunk_cols slots each),
    //   sync[PG_SYNC_DONE + b] = column slots of scratch buffer b whose posteriors are done, over all its chunks so far (k_post_loop)
    uint32_t* sync;            // [PG_SYNC_WORDS]
    uint32_t  chunk_cols;
    uint32_t  col_stride;      // doubles between consecutive columns of `fwd`: HP*HP, or 2304 (the 18 KB of a compact triangle) when tri
    uint8_t*  wide;            // wide entries (see above)
    const uint32_t* wide_idx;  // [V]: byte offset / 16 of the entry of variant v, PG_WIDE_NONE if it has <= PG_AMAX alleles
    uint8_t*  vpair;           // [V][pg_pair_bytes(pair_n)]
    // lean sweep (k_sweep_lean: HP = H = 64, every object biallelic): compact column records
    // {c0, c1, c2, kappa, E'00, E'01, E'11, bits1} (64 B, read with scalar loads) and the flag
    double*   frec;            // [V][8]
    // 1: every object of the chain is biallelic with at most 32 k-mers and H <= 64: k_prep_bi prepares four variants
    // per wave (a DPP row of 16 lanes each) instead of k_prep's one (PG_KERNELS=prepwave keeps k_prep: cross-check); 2: at least
    // half of the objects are such: k_prep_bi takes those, k_prep the others (each kernel skips the other's objects)
    uint32_t  prep_fast;
    // prep_fast == 2: the objects with 3 .. PG_AMAX alleles and <= 64 k-mers (k_prep_m4: four per wave) and every other object
    // that is not k_prep_bi's (k_prep: one per wave), as lists of variant ids per index contig — null: k_prep walks all variants
    uint32_t  n_prep_m4, n_prep_w;
    uint32_t  n_prep_b;        // ... and k_prep_bi's own objects (two alleles, <= 32 k-mers)
    const uint32_t* prep_m4;
    const uint32_t* prep_w;
    const uint32_t* prep_b;
    uint32_t  lean;            // 1: the store-only phases of this chain run on k_sweep_lean
    // 1 or 2 (lean chains of FUSED jobs; 2: phase 2 on k_sweep_lean2, 1: on the general kernel's triangle ring): phase 1 stores only the upper triangle of its (symmetric) columns, COMPACT at the
    // start of the column's slot (1152 16-byte units: row pair q, lanes 8 (q >> 2) .. 63, see tri_unit_of); elements
    // below the diagonal inside those units are written as 0, the diagonal is stored HALVED — so that phase 2 can
    // take the posterior sums over the stored half alone and k_bins doubles them: half the HBM bytes written by
    // phase 1 and read by phase 2
    uint32_t  tri;
    // 1 (tri == 1 and the chain is not a lean chain: 64 paths, multiallelic objects, fused job): phase 2 on k_sweep_leanx2 — the
    // posterior partials leave added up over the four waves, T = 64 entries per column and slot pair (PG_KERNELS=noleanx2: the
    // general kernel's triangle ring, T = 256)
    uint32_t  leanx2;
    // 1 (round 6, 64-path chains of FUSED jobs on the general kernel whose objects include wide ones — more than PG_AMAX alleles on the
    // selected paths): a wide column costs that column, not the job — its phase-2 role stores its own column P' / beta' in the
    // variant's aux slot (8 HP^2 bytes, PG_REC_AUX) instead of forming posterior partials, and k_bins_wide forms the bins from
    // that column and the stored partner (post_ab: what k_post does for every column of a chunked job).  PG_KERNELS=nowidef:
    // such a job runs chunked, as before.
    uint32_t  widef;
    // 1: every object of the chain is biallelic and H = HP = 16: the store-only phases run on k_sweep_small16 (four
    // half-chains per wave); the chain keeps its compact records (frec) next to the full ones
    // 2 (fused jobs, with cls4): phase 2 runs there too — partner columns prefetched into registers three steps ahead, the four
    // class sums of a column formed inside the 16-lane row
    uint32_t  small;
    // 1: HP = 128 or 64, every object has at most PG_AMAX alleles (all columns narrow) and the chain is not `lean`: the
    // store-only phases run on k_sweep_leanx (the lean step with table emissions)
    uint32_t  leanx;
    // 1 (fused jobs): HP = 16 or 32, H = HP, every object biallelic: phase 2 (general kernel, one compute wave per
    // half-chain) writes the four class sums of a column, part[4 c + 2 (row allele) + (column allele)], and
    // k_bins_lean2 turns them into bins — instead of per-thread partials reduced by k_bins
    uint32_t  cls4;
    // 1 / 2: HP = H = 16 and NOT every object biallelic: the store-only phases (1) / both phases (2: fused jobs) run on
    // k_sweep_small16x (pg_small16x.h): 192-byte column records in `frec`, class sums of columns with at most two local
    // alleles in `part` ([C][4]), the fifteen bins of columns with three to five and the phase-2 column of WIDE columns in
    // the variant's `aux` slot (k_bins_x, k_bins_wide)
    uint32_t  smallx;
    // 1 / 2 (small == 2 / smallx == 2 chains of fused jobs without run_phasing): the split path, see above
    uint32_t  split;
    const uint32_t* col_of;    // [V] per index contig: column of a kept variant, PG_COL_NONE otherwise
    const unsigned char* ix_pd;
    const unsigned char* ix_rec;
    const unsigned char* ix_bin;
    unsigned char* cprec;      // [V][192] per chain (touched for flagged columns only)
    uint32_t* ix_err;          // per index contig: error bits of k_index_scan (PG_DEVERR_*)
    const uint32_t* ix_big;    // per index contig: its variants with more than 32 alleles (the wave-per-object index kernels' list)
    uint32_t n_ix_big;
    // 1 (lean chains of chunked jobs that leave CUs idle, chunk_cols a multiple of PG_LEAN_SPARSE): phase 1 stores only every
    // PG_LEAN_SPARSE-th column, counted from the phase boundary (pg_sparse_*, below); k_refill_lean re-runs the columns between two
    // stored ones on the idle CUs, chunk by chunk, before k_post reads them (PG_KERNELS=nosparse: every column by the chain)
    uint32_t sparse;
    // 1 (sparse, and every chain of the job with columns is such a chain): the chunk sweeps of phase 2 store only their checkpoints
    // too (pg_sparse2_*, below) — into `ckpt`, an area of the chain's own that no run reuses, not into the scratch buffers: a chunk
    // sweep then neither stores its columns nor waits for k_post to free a buffer.  k_refill_lean forms the chunk's columns from the
    // checkpoints into the scratch slots k_post reads, behind the sweep on the second stream (PG_KERNELS=nosparse2: the chunk
    // sweeps store every column into the scratch buffers, as the chains of every other job do)
    uint32_t sparse2;
    uint32_t ckpt_slots;       // pg_sparse2_slots(V)
    double*  ckpt;             // [2 roles][ckpt_slots][64 * 64], forward role first: slot m = checkpoint m of the role's phase 2
    // the WIDE columns of the chain (smallx == 2, index with objects of more than PG_AMAX alleles): k_records appends every wide
    // column it meets, k_bins_wide walks the list — one wave per entry instead of a scan of all columns for the rare one
    uint32_t* wcols;           // [wide candidates of the index contig]
    uint32_t* n_wcols;         // (zeroed at the start of every run)
    unsigned char* aux;        // per chain: slots of the variants with more than two alleles (128 B) / more than PG_AMAX (8 HP^2 B)
    const uint32_t* aux_idx;   // [V] per index contig: byte offset / 16 of the variant's slot, PG_WIDE_NONE if it has two alleles
    // rows and lanes of a stored column that carry data: H rounded up to a multiple of 4 (fused jobs at HP = 32, where
    // 17 paths — a user-chosen panel size of 16 + the reference path; the DEFAULT, 15 + 1 = 16 paths, runs on k_sweep_small16[x] — would otherwise move 32 x 32 states per column for 17 x 17 real ones), else HP.
    // Phase 1 stores only rows and lanes below `live` (whole 64-byte sectors), the loader of phase 2 fetches only those,
    // and the rest of the LDS ring is zeroed once.  Nothing else reads the columns of a fused job.
    uint32_t  live;
    double*   xbuf;            // [2][HP*HP] generic kernel scratch (forward role first)
    uint32_t* err;
    unsigned long long* prof;  // [64] in-kernel cycle counters (-DPG_CHAIN_PROF / -DPG_LEAN_TIMELINE builds), profiling only
    // Viterbi phasing (run_phasing, pg_viterbi.hip): transition probabilities {p^2, pq, q^2} of every column,
    // the backtrace (index of the best previous state of every state, H*H per column), the best state of
    // the last column, and the haplotype alleles per variant
    double*   vit_tq;          // [V][8]: {t0, t1, t2} as exact (hi, lo) pairs of the long double values, formed on the host
    uint16_t* vit_back;        // [V][H][HP]: state index (p1 * H + p2) of the best previous state of state (p1, p2)
    uint32_t* vit_best;        // [1]
    uint16_t* hap1;            // [V] allele of the first / second haplotype at kept variants, 0 elsewhere
    uint16_t* hap2;
    // outputs
    double*   lik;             // [n_lik] mantissa in [0.5,1) or 0
    int32_t*  lik_exp;         // [n_lik] exponent: L = lik * 2^lik_exp
};

// ------------------------------------------------------------------------------------------------------------------
//  Sparse phase 1 of lean chains (DevContig::sparse): where the stored columns (checkpoints) lie and which columns a refill
//  segment re-runs.  Host and device take both from here.  With mid = C / 2 the forward role walks columns 0 .. mid-1 and
//  stores mid-1 - m S, the backward role walks C-1 .. mid and stores mid + m S (m = 0, 1, ...): the column phase 2 resumes
//  from is always stored, and with chunk_cols a multiple of S the partner columns of a chunk are whole segments.  The columns
//  in front of a role's first checkpoint (from column 0 / C-1, where the recursion is initialised) are stored by the chain.
//  Segment m >= 1 of a role resumes from checkpoint m and runs, in the role's own direction, the S - 1 columns up to
//  checkpoint m - 1.  Chunk i of phase 2 reads segments i q + 1 .. (i + 1) q of either role, q = chunk_cols / S.
// ------------------------------------------------------------------------------------------------------------------
#define PG_LEAN_SPARSE 64u
#ifdef __HIP__   // (the HIP translation units; pg_shim.cpp is host C++)
#define PG_HD __attribute__((host)) __attribute__((device))
#else
#define PG_HD
#endif
// segments a role has: checkpoints m = 1 .. this many exist
PG_HD inline uint32_t pg_sparse_segments(uint32_t C, uint32_t role) {
    const uint32_t mid = C / 2u;
    if (role == 0u) return mid ? (mid - 1u) / PG_LEAN_SPARSE : 0u;
    return C ? (C - 1u - mid) / PG_LEAN_SPARSE : 0u;
}
// column of checkpoint m (m <= pg_sparse_segments)
PG_HD inline uint32_t pg_sparse_checkpoint(uint32_t C, uint32_t role, uint32_t m) {
    const uint32_t mid = C / 2u;
    return role == 0u ? mid - 1u - m * PG_LEAN_SPARSE : mid + m * PG_LEAN_SPARSE;
}
// does the chain itself store column c of its phase-1 half (a checkpoint, or a column of the leading piece)?
PG_HD inline bool pg_sparse_stored(uint32_t C, uint32_t role, uint32_t c) {
    const uint32_t mid = C / 2u;
    if (role == 0u) return c >= mid || (mid - 1u - c) % PG_LEAN_SPARSE == 0u || c < (mid - 1u) % PG_LEAN_SPARSE;
    return c < mid || (c - mid) % PG_LEAN_SPARSE == 0u || c > mid + pg_sparse_segments(C, 1u) * PG_LEAN_SPARSE;
}
// Phase 1 in pieces (pg_job::pieces): a role's phase-1 columns whose partner chunk of phase 2 lies in [g G, (g + 1) G) are piece g,
// `piece_cols` = G chunk_cols columns (a multiple of S) counted from the phase boundary — one launch per piece, the farthest piece
// first, so that the partner columns of a piece's chunks can be refilled while the chain runs the pieces nearer the boundary.  The
// column in front of a piece (the last one of piece g + 1) is a checkpoint: the piece resumes from what the chain stored anyway.
// false: the role has no column that far from the boundary; out = {lowest column, highest column}
#define PG_PIECE_CHUNKS_DEFAULT 4u   // G (profiles/r11_refill_beside_phase1.txt); PG_PIECE_CHUNKS overrides it
PG_HD inline bool pg_sparse_piece(uint32_t C, uint32_t role, uint32_t piece_cols, uint32_t g, uint32_t out[2]) {
    const unsigned long long mid = C / 2u, half = role == 0u ? mid : C - mid;
    const unsigned long long d0 = (unsigned long long)g * piece_cols;   // columns between the piece and the phase boundary
    if (piece_cols == 0u || piece_cols % PG_LEAN_SPARSE != 0u || d0 >= half) return false;
    const unsigned long long d1 = half - d0 > piece_cols ? d0 + piece_cols : half;
    if (role == 0u) { out[0] = (uint32_t)(mid - d1); out[1] = (uint32_t)(mid - 1u - d0); }
    else { out[0] = (uint32_t)(mid + d0); out[1] = (uint32_t)(mid + d1 - 1u); }
    return true;
}
// The record ring of a sparse lean launch (pg_kernels.hip: LeanRecs, lean_forward / lean_backward in their SPARSE form).  The
// records of a launch are numbered along the role's direction and live in LDS in two blocks of S; step number n reads records
// n + 1 and n + 2, parks block (n + 4) / S when n + 4 is a multiple of S and expands block (n + 3) / S when n + 3 is.  A sparse
// launch runs `lead` storing steps (at most S - 1), then groups of S steps (S - 1 store-free, one storing), then — a chunk sweep
// of phase 3 — a tail.  Its first step takes the number pg_lean_ring_first(lead) instead of 0, so that the first step of every
// group has a number that is a multiple of S: inside a group the block is parked at step PG_LEAN_RING_PARK and expanded at step
// PG_LEAN_RING_EXPAND, the same in every group, and the other steps of a group are compiled without the two tests.  The records
// in front of the launch's first one that the numbering adds are fetched clamped and never read.  A first number of
// PG_LEAN_RING_PARK + 1 or more starts behind the step that would park block 1: the launch parks and expands it up front.
// What a step reads of record `rel` lies in ONE image of PG_LEAN_IMAGE bytes (LeanShared::img: the compact record, its pair table
// and its pair bytes at fixed offsets), the ring of 2 S images in record order: pg_lean_ring_image is the image's byte offset.
#define PG_LEAN_IMAGE 256u
PG_HD inline uint32_t pg_lean_ring_image(uint32_t rel) { return (rel * PG_LEAN_IMAGE) & (2u * PG_LEAN_SPARSE * PG_LEAN_IMAGE - 1u); }
#define PG_LEAN_RING_PARK (PG_LEAN_SPARSE - 4u)
#define PG_LEAN_RING_EXPAND (PG_LEAN_SPARSE - 3u)
PG_HD inline uint32_t pg_lean_ring_first(uint32_t lead) { return (PG_LEAN_SPARSE - lead % PG_LEAN_SPARSE) % PG_LEAN_SPARSE; }
// steps of a sparse launch in front of its first group: `c0` = column of the launch's first step; `end` = forward, one past the
// column of its last step (the steps run c0 .. end - 1); backward, the column of its last step (c0 down to end).  Phase 3 starts
// on a group.
PG_HD inline uint32_t pg_lean_ring_lead(uint32_t C, uint32_t role, uint32_t phase, uint32_t c0, uint32_t end) {
    if (phase != 1u) return 0u;
    if (role == 0u) { const uint32_t ck0 = end ? (end - 1u) % PG_LEAN_SPARSE : 0u; return c0 <= ck0 ? ck0 - c0 + 1u : 0u; }
    const unsigned long long ckh = (unsigned long long)(C / 2u) + (unsigned long long)pg_sparse_segments(C, 1u) * PG_LEAN_SPARSE;   // the first checkpoint on the way down
    return c0 >= ckh ? (uint32_t)(c0 - ckh) + 1u : 0u;
}
// A sparse launch as the kernels walk it: phase 1 (chunk = 0: the whole half; G << 16 | g: piece g of G chunks) or a chunk sweep
// of phase 3 (chunk = its number).  false: no step.  out = {column of the first step, number of steps, lead}
PG_HD inline bool pg_lean_ring_launch(uint32_t C, uint32_t role, uint32_t phase, uint32_t K, uint32_t chunk, uint32_t out[3]) {
    const unsigned long long mid = C / 2u;
    if (role == 0u) {
        unsigned long long lo = phase == 1u ? 0u : mid, hi = phase == 1u ? mid : C;
        if (phase == 3u) { lo = mid + (unsigned long long)chunk * K; if (lo >= C) return false; hi = C - lo > K ? lo + K : C; }
        if (phase == 1u && chunk) { uint32_t pc[2]; if (!pg_sparse_piece(C, 0u, (chunk >> 16) * K, chunk & 0xFFFFu, pc)) return false; lo = pc[0]; hi = pc[1] + 1ull; }
        const unsigned long long first = lo == 0u ? 1u : lo;
        if (first >= hi) return false;
        out[0] = (uint32_t)first; out[1] = (uint32_t)(hi - first); out[2] = pg_lean_ring_lead(C, 0u, phase, (uint32_t)first, (uint32_t)hi);
        return true;
    }
    if (C == 0u) return false;
    long long top = phase == 1u ? (long long)C - 1 : (long long)mid - 1, bot = phase == 1u ? (long long)mid : 0;
    if (phase == 3u) { top = (long long)mid - 1 - (long long)chunk * K; if (top < 0) return false; bot = top - (long long)K + 1 > 0 ? top - (long long)K + 1 : 0; }
    bool resumed = phase != 1u;
    if (phase == 1u && chunk) { uint32_t pc[2]; if (!pg_sparse_piece(C, 1u, (chunk >> 16) * K, chunk & 0xFFFFu, pc)) return false; bot = pc[0]; top = pc[1]; resumed = top != (long long)C - 1; }
    const long long t0 = resumed ? top : top - 1;
    if (t0 < bot) return false;
    out[0] = (uint32_t)t0; out[1] = (uint32_t)(t0 - bot + 1); out[2] = pg_lean_ring_lead(C, 1u, phase, (uint32_t)t0, (uint32_t)bot);
    return true;
}
// The preparation beside phase 1 (pg_job::prep_beside; pg_shim_run.cpp: prepare_in_parts): a job whose phase 1 runs in pieces
// prepares only what its first E pieces read ahead of them — the ENDS of the chains — and the rest, the MIDDLE, on the second
// stream beside those pieces.  The middle of a chain of C columns is one band around the phase boundary, W = (n_pieces - E)
// piece_cols columns (a multiple of S) to either side of it: columns [out[0], out[1]).  Pieces 0 .. n_pieces - E - 1 of either
// role lie inside it, every column of a later piece outside; W at least a half: the whole chain is middle.
#define PG_PREP_EARLY_PIECES_DEFAULT 2u   // E (PG_PREP_EARLY_PIECES overrides it)
PG_HD inline uint32_t pg_prep_band(uint32_t n_pieces, uint32_t E, uint32_t piece_cols) {   // W (n_pieces > E); capped: no half is wider
    const unsigned long long W = (unsigned long long)(n_pieces - E) * piece_cols;
    return W > 0xFFFFFFC0ull ? 0xFFFFFFC0u : (uint32_t)W;
}
PG_HD inline void pg_prep_middle(uint32_t C, uint32_t W, uint32_t out[2]) {
    const uint32_t mid = C / 2u;
    out[0] = mid - (mid < W ? mid : W);
    out[1] = mid + (C - mid < W ? C - mid : W);
}
// ... and of its V variants: a variant goes with its column, a variant that is no column with the next column below it (the
// variants below the first column: with column 0) — read off col_variant, which ascends, at the band's two edges: variants
// [out[0], out[1]).  No column: the whole chain is middle.
PG_HD inline void pg_prep_middle_variants(const uint32_t* col_variant, uint32_t C, uint32_t V, uint32_t W, uint32_t out[2]) {
    uint32_t cr[2];
    pg_prep_middle(C, W, cr);
    out[0] = cr[0] == 0u ? 0u : col_variant[cr[0]];
    out[1] = cr[1] >= C ? V : col_variant[cr[1]];
}
// item `u` of a part of N items (columns or variants) whose middle is [lo, hi): part 2 is the middle in order, part 1 the ends
// — what lies below the middle, then what lies above it.  N: the part has no item u.
PG_HD inline uint32_t pg_prep_part_item(uint32_t part, uint32_t lo, uint32_t hi, uint32_t N, uint32_t u) {
    if (part == 2u) return u < hi - lo ? lo + u : N;
    return u < lo ? u : (u < N - (hi - lo) ? u + (hi - lo) : N);
}

// ------------------------------------------------------------------------------------------------------------------
//  Sparse phase 2 (DevContig::sparse2): the checkpoints go on in phase 1's step from the phase boundary — the forward role walks
//  mid .. C-1 and stores mid-1 + m S, the backward role walks mid-1 .. 0 and stores mid - m S (m = 1, 2, ...; checkpoint 0 is
//  phase 1's: fwd[mid-1] / fwd[mid]).  With chunk_cols a multiple of S the last column of every chunk is a checkpoint: the next
//  chunk launch resumes from it.  Segment m >= 0 of a role resumes from checkpoint m and runs, in the role's own direction, the
//  S columns up to and including checkpoint m + 1 — fewer at the end of the half, whose last piece the chain does not store
//  either.  Chunk i of phase 2 is segments i q .. (i + 1) q - 1 of either role, q = chunk_cols / S.
// ------------------------------------------------------------------------------------------------------------------
PG_HD inline uint32_t pg_sparse2_slots(uint32_t V) { return (V / 2u + 1u) / PG_LEAN_SPARSE + 2u; }   // (a half has at most V / 2 + 1 columns)
// segment m of a role: false if it has no columns; out = {checkpoint it resumes from, its lowest column, its highest column}
PG_HD inline bool pg_sparse2_segment(uint32_t C, uint32_t role, unsigned long long m, uint32_t out[3]) {
    if (C < 2u) return false;   // (a single column is the forward role's initial one: no checkpoint in front of it)
    const unsigned long long mid = C / 2u, d = m * PG_LEAN_SPARSE;
    if (role == 0u) {
        const unsigned long long ck = mid - 1u + d;
        if (ck + 1u >= C) return false;
        out[0] = (uint32_t)ck; out[1] = (uint32_t)ck + 1u; out[2] = (uint32_t)(C - 1u - ck > PG_LEAN_SPARSE ? ck + PG_LEAN_SPARSE : C - 1u);
    } else {
        if (d >= mid) return false;
        const unsigned long long ck = mid - d;
        out[0] = (uint32_t)ck; out[1] = (uint32_t)(ck > PG_LEAN_SPARSE ? ck - PG_LEAN_SPARSE : 0u); out[2] = (uint32_t)ck - 1u;
    }
    return true;
}
// does the chain itself store column c of its phase-2 half (a checkpoint)?
PG_HD inline bool pg_sparse2_stored(uint32_t C, uint32_t role, uint32_t c) {
    const uint32_t mid = C / 2u;
    if (C < 2u) return false;
    if (role == 0u) return c >= mid && c < C && (c - (mid - 1u)) % PG_LEAN_SPARSE == 0u;
    return c < mid && (mid - c) % PG_LEAN_SPARSE == 0u;
}

// ------------------------------------------------------------------------------------------------------------------
//  The seam between the count plan (pg_kmers.hip owns the counter and the plan) and a cohort job (pg_shim.cpp owns pg_job):
//  pg_count_plan_fill_job (include/pangenie_counts.h) writes one sample's arrays straight into the job.  Internal: not
//  part of any public header, not exported.
//   _begin: checks (cohort job on `device`, no upload in flight, sample in range, contig c has n_variants[c] and
//           kmer_off[c]), makes `stream` (a hipStream_t) wait for the job's stream, and answers the device arrays of chains
//           sample * n_contigs + c inside the set the next pg_job_run reads.
//   _end:   the job's stream waits for `stream`, coverage[c] (host, n_variants[c] entries) becomes the host copy of those
//           chains' coverage, and the results of the last run are invalidated (as pg_job_upload_end does).
struct pg_job;
extern "C" {
__attribute__((visibility("hidden"))) int pgi_job_fill_begin(struct pg_job* job, uint32_t sample, int device, uint32_t n_contigs, const uint32_t* n_variants,
                                                            const uint32_t* const* kmer_off, void* stream, uint16_t** d_kmer_count, uint16_t** d_coverage,
                                                            char* err, size_t errlen);
__attribute__((visibility("hidden"))) int pgi_job_fill_end(struct pg_job* job, uint32_t sample, uint32_t n_contigs, const uint16_t* const* coverage, void* stream,
                                                          char* err, size_t errlen);
}
