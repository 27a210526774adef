// pg_shim_run.cpp — pg_job_run: the run schedule of a job, as a list of named steps (DESIGN.md §4 "The run schedule, step by
// step" maps each step to the section that explains it).  A run is: settle a pipelined upload, zero the per-run block, prepare
// (whole, or in parts: the ends of the chains ahead, their middle on the second stream beside the first pieces of phase 1),
// phase 1, ONE of four phase 2s (fused / persistent / sparse / chunks), the Viterbi, one wait, timings and error bits.  Every
// step says what it reads of the job and which streams it touches; `s` is the run's stream (the caller's, or the job's own),
// "second" is pg_job::stream2.  Which schedule a job takes was decided when it was built (job_build, pg_shim.cpp); a run adds
// three facts of its own: is a pipelined upload still in flight (pg_job::late_pending), is `s` the job's own stream, and do
// the two streams run side by side (streams_concurrent).  pg_shim.cpp keeps the build and the uploads; both see pg_job.h.
#include <hip/hip_runtime_api.h>

#include <math.h>

#include <algorithm>
#include <vector>

#include "pg_job.h"

using namespace pgj;

#define STEP(call)                        \
    do {                                  \
        const int rc_ = (call);           \
        if (rc_ != PG_OK) return rc_;     \
    } while (0)

namespace pgj __attribute__((visibility("hidden"))) {
// The persistent phase 2 needs the kernels of `s` and of the job's second stream to run SIDE BY SIDE (they wait for each other).
// Streams are mapped onto a few hardware queues, and two streams on one queue run one after the other: ask the device once per
// stream (k_stream_handshake); a second stream that shares the queue is replaced by a new one, a few times.  False: this run
// takes a launch per chunk.
bool streams_concurrent(pg_job* job, hipStream_t s) {
    if (job->persist_checked_any && job->persist_checked == s) return true;
    for (int attempt = 0; attempt < 6; ++attempt) {
        uint32_t w[4] = {0, 0, 0, 0};
        if (hipMemcpyAsync(job->d_handshake, w, sizeof(w), hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) break;
        pgk_launch_stream_handshake(job->d_handshake, s, job->stream2);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipStreamSynchronize(job->stream2) != hipSuccess) break;
        if (hipMemcpy(w, job->d_handshake, sizeof(w), hipMemcpyDeviceToHost) != hipSuccess) break;
        if (w[2] == 1u) { job->persist_checked = s; job->persist_checked_any = true; return true; }
        hipStream_t fresh = nullptr;   // (created BEFORE the old one is destroyed: the runtime hands a new stream the least used queue)
        if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) break;
        (void)hipStreamDestroy(job->stream2);
        job->stream2 = fresh;
    }
    (void)hipGetLastError();
    return false;
}
}  // namespace pgj

namespace {

// What one run found out and its later steps read.
struct RunPlan {
    bool genotype = false;      // the job has variants and run_genotyping is on
    bool index_b_due = false;   // a pipelined upload was settled for a caller's stream: group B's index pass is made up in `prepare`
    bool persist_now = false;   // this run's phase 2 is the persistent one
    bool pieces_now = false;    // this run's phase 1 went in pieces: the second stream has refilled the partner columns of all chunks but piece 0's
    bool prep_beside_now = false;   // this run prepares the middle of the chains on the second stream, beside the first pieces of phase 1
};

// Group B's copy threads are joined and their return codes looked at.  Reads late_threads, late_rc; touches no stream.
int join_late_checked(pg_job* job, char* err, size_t errlen) {
    join_late_threads(job);
    for (int rcb : job->late_rc)
        if (rcb != (int)hipSuccess) { set_err(err, errlen, "input upload: %s", hipGetErrorString((hipError_t)rcb)); return PG_ERR_DEVICE; }
    return PG_OK;
}

// A pipelined upload followed by a run on a CALLER's stream: no pipelining — group B's inputs are waited for NOW, before
// streams_concurrent may replace the second stream, which their copies are on; `s` waits for the copies, group B's index pass is
// made up in `prepare` (plan->index_b_due).  NO CALLER IN THE TREE REACHES THIS: pg_job::pipeline is armed only inside calls that
// run the job themselves with a null stream (job_build with cache_arena, pg_job_upload_run).  Kept on purpose: what a pipelined
// upload leaves in flight must not hang on who runs the job next.
// Reads late_pending, ev_late[1]; streams: second (record), s (wait).
int settle_late_for_callers_stream(pg_job* job, hipStream_t s, RunPlan* plan, char* err, size_t errlen) {
    plan->index_b_due = job->late_pending && s != job->stream;
    if (!plan->index_b_due) return PG_OK;
    STEP(join_late_checked(job, err, errlen));
    HIP_TRY(hipEventRecord(job->ev_late[1], job->stream2));
    HIP_TRY(hipStreamWaitEvent(s, job->ev_late[1], 0));
    return PG_OK;
}

// The pipelined first run (pg_job::pipeline): group A's preparation and phase 1 start NOW, on `s`; the host then waits for
// group B's inputs (they have been crossing PCIe since job_build) and puts B's index pass, preparation and phase 1 on the
// second stream, beside A's.  Phase 2 starts when both are done.  (The timing classes: B's preparation counts into the
// phase-1 class.)
// Reads nA, d_contigs_g, d_reps_g, the prep extents, hp_mask; streams: s (group A), second (group B), joined by ev_late[0 / 1].
int first_run_pipelined(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size(), nA = job->nA, nB = n - nA;
    HIP_TRY(hipEventRecord(job->ev_late[0], s));   // (behind the zeroing of the per-run block)
    pgk_launch_prep(job->d_contigs_g, nA, job->max_v, job->max_prep_w, job->max_prep_m4, job->tab, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[1], s));
    HIP_TRY(hipEventRecord(job->ev[2], s));
    pgk_launch_records(job->d_contigs_g, nA, job->max_v, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[3], s));
    pgk_launch_sweep(job->d_contigs_g, nA, job->hp_mask, 1, s);
    HIP_TRY(hipGetLastError());
    STEP(join_late_checked(job, err, errlen));   // (their copies are ISSUED — 17 ms on the whole genome —, on stream2)
    hipStream_t sb = job->stream2;
    HIP_TRY(hipStreamWaitEvent(sb, job->ev_late[0], 0));
    pgk_launch_index(job->d_reps_g + nA, nB, job->max_v, max_big_list(job), 0, sb);
    pgk_launch_prep(job->d_contigs_g + nA, nB, job->max_v, job->max_prep_w, job->max_prep_m4, job->tab, sb);
    pgk_launch_records(job->d_contigs_g + nA, nB, job->max_v, sb);
    pgk_launch_sweep(job->d_contigs_g + nA, nB, job->hp_mask, 1, sb);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_late[1], sb));
    HIP_TRY(hipStreamWaitEvent(s, job->ev_late[1], 0));
    HIP_TRY(hipEventRecord(job->ev[4], s));
    return PG_OK;
}

// Group B's index pass where a settled pipelined upload left it out, then the emission tables and the variant records as ever.
// Reads any_legacy_prep, any_split, the prep extents, tab; stream: s alone.  Records ev[1 .. 3].
int prepare(pg_job* job, hipStream_t s, bool index_b_due, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    if (index_b_due) {
        pgk_launch_index(job->d_reps_g + job->nA, n - job->nA, job->max_v, max_big_list(job), 0, s);
        HIP_TRY(hipGetLastError());
    }
    if (job->any_legacy_prep) pgk_launch_prep(job->d_contigs, n, job->max_v, job->max_prep_w, job->max_prep_m4, job->tab, s);
    if (job->any_split) pgk_launch_prep_split(job->d_contigs, n, job->max_sb, job->max_sm4, job->max_sw, job->tab, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[1], s));
    // (no k_compact: the column list is the index's, made when it was uploaded — the class stays in the timing table, at zero)
    HIP_TRY(hipEventRecord(job->ev[2], s));
    if (job->any_legacy_prep) pgk_launch_records(job->d_contigs, n, job->max_v, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[3], s));
    return PG_OK;
}

// The grid extents of the two parts of a preparation in parts (pg_job::prep_beside): the most variants / columns a chain has in
// its ends and in its middle, from the column counts and the two column-list entries at the edges of every index contig's middle
// (pg_device.h: pg_prep_middle, pg_prep_middle_variants).  They hang on the index alone: read once per uploaded index, by the
// first such run — nothing is in flight on either stream then (an upload and a run both return synchronised).
// Reads prep_W, d.n_cols, d.col_variant; touches no stream (blocking copies).
int prep_part_extents(pg_job* job, char* err, size_t errlen) {
    if (job->prep_parts_ready) return PG_OK;
    std::vector<char> done(job->index.size(), 0);
    uint32_t mv[2] = {0, 0}, mc[2] = {0, 0};
    for (const ChainHost& ch : job->chains) {
        const IndexHost& x = job->index[ch.index];
        if (x.V == 0 || done[ch.index]) continue;
        done[ch.index] = 1;
        uint32_t C = 0, cr[2], vr[2] = {0u, x.V};
        HIP_TRY(hipMemcpy(&C, ch.d.n_cols, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (C > x.V) { set_err(err, errlen, "index contig %u: bad column count", ch.index); return PG_ERR_DEVICE; }
        pg_prep_middle(C, job->prep_W, cr);
        if (cr[0] > 0u) HIP_TRY(hipMemcpy(&vr[0], ch.d.col_variant + cr[0], sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (cr[1] < C) HIP_TRY(hipMemcpy(&vr[1], ch.d.col_variant + cr[1], sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (vr[0] > vr[1] || vr[1] > x.V) { set_err(err, errlen, "index contig %u: bad column list", ch.index); return PG_ERR_DEVICE; }
        mc[0] = std::max(mc[0], C - (cr[1] - cr[0])); mc[1] = std::max(mc[1], cr[1] - cr[0]);
        mv[0] = std::max(mv[0], x.V - (vr[1] - vr[0])); mv[1] = std::max(mv[1], vr[1] - vr[0]);
    }
    for (int p = 0; p < 2; ++p) { job->prep_max_v[p] = mv[p]; job->prep_max_c[p] = mc[p]; }
    job->prep_parts_ready = true;
    return PG_OK;
}

// The preparation in parts (pg_job::prep_beside: phase 1 in pieces, k_prep_bi the job's only emission kernel; this run on the
// job's own stream, no pipelined upload in flight).  Part 1, the ENDS of the chains — every column farther than prep_W from the
// phase boundary, all that the first prep_early pieces step through — on `s`, in front of phase 1 as ever; part 2, the MIDDLE,
// on the second stream beside those pieces, behind ev[3] — that is behind the per-run zeroing (ev[0]), which clears the error bits
// part 2 writes, AND behind part 1: started at ev[0], part 2's forty thousand workgroups took the chip from part 1's thousand, and
// the first piece waited 0.7 – 2.3 ms for them instead of 0.1 (profiles/r17_prep_beside_phase1.txt).  ev_prep2 says part 2 is done.
//  * Who reads what part 2 writes (vrec, vpair, kept, allele_present; the compact records, frec): the pieces from
//    n_pieces - prep_early - 1 down, the chunk sweeps and the Viterbi on `s` — all behind the wait for ev_prep2 in phase1_in_pieces;
//    every refill, k_post and part 2 itself on the second stream — in stream order behind part 2.
//  * Read-ahead: a piece fetches compact records up to two 64-column blocks past its last column (LeanRecs::fetch; parked and
//    expanded in LDS) and reads the record and the emissions of the column behind its last one into registers a step ahead — but a
//    forward step's column t is formed from the records of columns <= t and a backward step's from those of columns >= t
//    (lean_forward / lean_backward: `cur`, `ec`; what is read ahead is used by the NEXT step alone, and the zero test that ends a
//    piece reads its last column's sums).  The last column of the last early piece is an end column, so no record of the middle
//    is consumed before the wait: the ends need no widening.  The refills behind the early pieces re-run columns of those pieces.
//  * Two runs of a resident job: part 2 of run n + 1 must not overtake the readers of run n (k_post, the Viterbi).  pg_job_run
//    returns with both streams synchronised — that orders the runs; a run that failed half way leaves k_post in front of part 2 in
//    the second stream's own order, and the Viterbi in front of ev[0] on `s`.
// The k_prep and k_records classes (ev[1 .. 3]) time part 1 alone; part 2 runs inside the span of the phase-1 class.
// Reads prep_W, prep_max_v / _c, tab, ev_prep2; streams: s (part 1), second (part 2; waits for ev[3]).  Records ev[1 .. 3].
int prepare_in_parts(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size(), W = job->prep_W;
    hipStream_t s2 = job->stream2;
    pgk_launch_prep_part(job->d_contigs, n, 1u, W, job->prep_max_v[0], job->tab, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[1], s));
    HIP_TRY(hipEventRecord(job->ev[2], s));
    pgk_launch_records_part(job->d_contigs, n, 1u, W, job->prep_max_c[0], s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[3], s));
    HIP_TRY(hipStreamWaitEvent(s2, job->ev[3], 0));
    pgk_launch_prep_part(job->d_contigs, n, 2u, W, job->prep_max_v[1], job->tab, s2);
    pgk_launch_records_part(job->d_contigs, n, 2u, W, job->prep_max_c[1], s2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_prep2, s2));
    return PG_OK;
}

// phase 1 in pieces (all chains sparse lean chains; the job's own stream, not the pipelined first run): piece g, then on the
// second stream the partner columns of its chunks, the farthest chunk first — a segment resumes from a checkpoint of its own
// piece or from the last column of the piece before, both stored by then.  Piece 0's chunks stay with phase 2
// `beside` (prepare_in_parts): the middle of the chains is being prepared on the second stream — `s` waits for it (ev_prep2) in front
// of piece n_pieces - prep_early - 1, the first that can step into the middle and the first in which a chain without ends starts;
// the refills behind the earlier pieces are behind part 2 in the second stream's order.
// Reads n_pieces, piece_chunks, n_chunks, chunk_cols, piece_refill_blocks, hp_mask, ev_piece, prep_early, ev_prep2; streams: s (pieces), second (refills).
int phase1_in_pieces(pg_job* job, hipStream_t s, bool beside, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size(), G = job->piece_chunks;
    const uint32_t others = job->hp_mask & ~PG_SWEEP_LEAN;   // (kernels of chains without columns: the launches they had — behind the wait, like every reader)
    if (others && !beside) pgk_launch_sweep(job->d_contigs, n, others, 1, s);
    for (uint32_t g = job->n_pieces; g-- > 0u;) {
        if (beside && g + 1u + job->prep_early == job->n_pieces) {
            HIP_TRY(hipStreamWaitEvent(s, job->ev_prep2, 0));
            if (others) pgk_launch_sweep(job->d_contigs, n, others, 1, s);
        }
        pgk_launch_sweep_piece(job->d_contigs, n, G, g, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_piece[g], s));
        if (g == 0u) break;
        HIP_TRY(hipStreamWaitEvent(job->stream2, job->ev_piece[g], 0));
        for (uint32_t i = std::min((g + 1u) * G, job->n_chunks); i-- > g * G;) pgk_launch_refill(job->d_contigs, n, job->chunk_cols, i, 0, job->piece_refill_blocks, job->stream2);
        HIP_TRY(hipGetLastError());
    }
    return PG_OK;
}

// Phase 1: in pieces (a job of more than one piece, on its OWN stream: a caller's stream gets the one launch, and phase 2
// refills every chunk) or as one launch; then the small sweeps.  Sets plan->pieces_now, records ev[4].
// Reads hp_mask, d_small / d_smallx, d_dump; stream: s (and what phase1_in_pieces touches).
int phase1(pg_job* job, hipStream_t s, RunPlan* plan, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    plan->pieces_now = job->n_pieces > 1u && s == job->stream;
    if (plan->pieces_now) STEP(phase1_in_pieces(job, s, plan->prep_beside_now, err, errlen));
    else pgk_launch_sweep(job->d_contigs, n, job->hp_mask, 1, s);
    pgk_launch_sweep_small(job->d_contigs, job->d_small, job->n_small, 1, 0, job->d_dump, s);
    pgk_launch_sweep_smallx(job->d_contigs, job->d_smallx, job->n_smallx, 1, 0, job->d_dump, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[4], s));
    return PG_OK;
}

// Fused phase 2: the sweeps form the posterior partials inline, k_bins reduces them.
// Reads hp_mask, small_phase2, smallx_phase2, bins_which, max_wide; stream: s alone.  Records ev[5], ev[6].
int phase2_fused(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    pgk_launch_sweep(job->d_contigs, n, job->hp_mask, 2, s);
    if (job->small_phase2) pgk_launch_sweep_small(job->d_contigs, job->d_small, job->n_small, 2, 0, job->d_dump, s);
    if (job->smallx_phase2) pgk_launch_sweep_smallx(job->d_contigs, job->d_smallx, job->n_smallx, 2, 0, job->d_dump, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[5], s));
    pgk_launch_bins(job->d_contigs, n, job->max_v, job->bins_which, job->max_wide, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev[6], s));
    return PG_OK;
}

// The end of every chunked phase 2, `s` having waited for the second stream's last posteriors.
int end_chunked_phase2(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    HIP_TRY(hipEventRecord(job->ev[5], s));  // "k_sweep_phase2" = all chunks incl. their posteriors
    HIP_TRY(hipEventRecord(job->ev[6], s));  // (no k_bins in this mode)
    return PG_OK;
}

// Persistent phase 2 — one launch each: the chunks are handed over on the device (DevContig::sync, zeroed with the per-run
// block); k_post_loop must not start (and wait) before phase 1 has ended.
// Reads post_blocks, ev[4], ev_post[0]; streams: s (sweep), second (k_post_loop; waits for ev[4]), s waits for ev_post[0].
int phase2_persistent(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    hipStream_t s2 = job->stream2;
    HIP_TRY(hipStreamWaitEvent(s2, job->ev[4], 0));
    pgk_launch_phase2_persistent(job->d_contigs, n, job->post_blocks, s, s2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_post[0], s2));
    HIP_TRY(hipStreamWaitEvent(s, job->ev_post[0], 0));
    return end_chunked_phase2(job, s, err, errlen);
}

// sparse phase 2: the chunk sweeps store their checkpoints into an area of their own and touch no scratch buffer — they
// wait for nothing.  The second stream forms chunk i's columns behind sweep i (k_refill_lean from those checkpoints) and
// then its posteriors: it writes and reads the scratch buffers alone, in order, so their rotation needs no event
// Reads n_chunks, chunk_cols, piece_chunks, hp_mask, ev_chunk, plan.pieces_now (phase 1 in pieces left only piece 0's partner
// columns to refill); streams: s (sweeps), second (refills, k_post; waits for ev[4] and every ev_chunk), s waits for ev_post[0].
int phase2_sparse(pg_job* job, hipStream_t s, const RunPlan& plan, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    hipStream_t s2 = job->stream2;
    if (job->sparse) HIP_TRY(hipStreamWaitEvent(s2, job->ev[4], 0));   // (the partner refills need phase 1 ended: see phase2_chunks)
    for (uint32_t i = 0; i < job->n_chunks; ++i) {
        pgk_launch_sweep_chunk(job->d_contigs, n, job->hp_mask, i, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_chunk[i], s));
        if (!plan.pieces_now || i < job->piece_chunks) pgk_launch_refill(job->d_contigs, n, job->chunk_cols, i, 0, 0u, s2);
        HIP_TRY(hipStreamWaitEvent(s2, job->ev_chunk[i], 0));
        pgk_launch_refill(job->d_contigs, n, job->chunk_cols, i, 1, 0u, s2);
        pgk_launch_post(job->d_contigs, n, job->chunk_cols, i, s2);
        HIP_TRY(hipGetLastError());
        if (i + 1u == job->n_chunks) {
            HIP_TRY(hipEventRecord(job->ev_post[0], s2));
            HIP_TRY(hipStreamWaitEvent(s, job->ev_post[0], 0));
        }
    }
    return end_chunked_phase2(job, s, err, errlen);
}

// Dense chunks, and chunks with sparse phase 1 —
// chunk i: store-only sweep on s -> ev_sweep -> k_post on stream2 -> ev_post; the sweep of chunk
// i + PG_SCRATCH_BUFS reuses scratch buffer i % PG_SCRATCH_BUFS and therefore waits for the posteriors of chunk i
// Reads n_chunks, chunk_cols, hp_mask, sparse, d_small / d_smallx, ev_sweep, ev_post; streams: s (sweeps), second (refills of a
// sparse phase 1, k_post), each waiting for the other's events; at the end s waits for the posteriors still out.
int phase2_chunks(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    hipStream_t s2 = job->stream2;
    // sparse phase 1: the refill of chunk i's partner columns (k_refill_lean) goes in front of k_post(i) on the second stream —
    // beside the sweep of chunk i, behind the posteriors of chunk i - 1; it needs phase 1 ended, nothing else
    if (job->sparse) HIP_TRY(hipStreamWaitEvent(s2, job->ev[4], 0));
    for (uint32_t i = 0; i < job->n_chunks; ++i) {
        const int b = (int)PG_SCR_BUF(i);
        if (i >= PG_SCRATCH_BUFS) HIP_TRY(hipStreamWaitEvent(s, job->ev_post[b], 0));
        pgk_launch_sweep_chunk(job->d_contigs, n, job->hp_mask, i, s);
        pgk_launch_sweep_small(job->d_contigs, job->d_small, job->n_small, 3, i, job->d_dump, s);
        pgk_launch_sweep_smallx(job->d_contigs, job->d_smallx, job->n_smallx, 3, i, job->d_dump, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_sweep[b], s));
        if (job->sparse) pgk_launch_refill(job->d_contigs, n, job->chunk_cols, i, 0, 0u, s2);
        HIP_TRY(hipStreamWaitEvent(s2, job->ev_sweep[b], 0));
        pgk_launch_post(job->d_contigs, n, job->chunk_cols, i, s2);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(job->ev_post[b], s2));
    }
    for (uint32_t q = 0; q < PG_SCRATCH_BUFS && q < job->n_chunks; ++q) HIP_TRY(hipStreamWaitEvent(s, job->ev_post[q], 0));
    return end_chunked_phase2(job, s, err, errlen);
}

// run_genotyping == false: the variant records (what the Viterbi reads; the column list is the index's).  Stream: s alone.
int records_only(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    pgk_launch_prep(job->d_contigs, (uint32_t)job->chains.size(), job->max_v, job->max_prep_w, job->max_prep_m4, job->tab, s);
    HIP_TRY(hipGetLastError());
    return PG_OK;
}

// Transition probabilities of the Viterbi, per kept column, formed on the host in long double exactly as the
// reference forms them (TransitionProbabilityComputer, src/transitionprobabilitycomputer.cpp:8-19, :33-39) and split
// into exact (hi, lo) double pairs: {t0, t1, t2} = {p^2, pq, q^2}.  The reference's decisions hang on p/q - 1, which
// drops below fp64's resolution once distance / H > 37 (pg_viterbi.hip).  Column 0 has no predecessor.
int viterbi_transitions(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    std::vector<std::vector<double>> tq_of_index(job->index.size());
    std::vector<char> done(job->index.size(), 0);
    std::vector<uint32_t> colv;
    for (uint32_t c = 0; c < n; ++c) {
        const ChainHost& ch = job->chains[c];
        const IndexHost& x = job->index[ch.index];
        if (x.V == 0) continue;
        std::vector<double>& tq = tq_of_index[ch.index];
        if (!done[ch.index]) {  // (the kept columns depend on the index alone: once per index contig)
            done[ch.index] = 1;
            uint32_t C = 0;
            HIP_TRY(hipMemcpy(&C, ch.d.n_cols, sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (C > x.V) { set_err(err, errlen, "chain %u: bad column count", c); return PG_ERR_DEVICE; }
            colv.resize(C ? C : 1);
            if (C) HIP_TRY(hipMemcpy(colv.data(), ch.d.col_variant, (size_t)C * sizeof(uint32_t), hipMemcpyDeviceToHost));
            tq.assign((size_t)C * 8, 0.0);
            const long double H = (long double)x.H;
            for (uint32_t k = 0; k < C; ++k) {
                long double t[3] = {1.0L, 1.0L, 1.0L};
                if (k > 0 && !job->params.uniform) {
                    const long double distance = (x.pos[colv[k]] - x.pos[colv[k - 1]]) * 0.000004L * ((long double)job->params.recombrate) * job->params.effective_N;
                    const long double recomb_prob = (1.0L - expl(-distance / H)) * (1.0L / H);
                    const long double no_recomb_prob = expl(-distance / H) + recomb_prob;
                    t[0] = no_recomb_prob * no_recomb_prob; t[1] = no_recomb_prob * recomb_prob; t[2] = recomb_prob * recomb_prob;
                }
                for (int q = 0; q < 3; ++q) {
                    const double hi = (double)t[q];
                    tq[(size_t)k * 8 + 2 * q] = hi;
                    tq[(size_t)k * 8 + 2 * q + 1] = (double)(t[q] - (long double)hi);  // exact: 64 - 53 bits are left
                }
            }
        }
        if (!tq.empty()) HIP_TRY(hipMemcpyAsync(ch.d.vit_tq, tq.data(), tq.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));  // (tq_of_index goes out of scope)
    return PG_OK;
}

// Viterbi phasing (reference src/hmm.cpp:47-49): reads k_prep's records, independent of the sweep
// Reads vit_tq_ready, vit_bits, ev_vit; stream: s — the first run with an index waits for BOTH streams, then uploads the
// transition probabilities of the kept columns.
int phase_viterbi(pg_job* job, hipStream_t s, char* err, size_t errlen) {
    if (!job->vit_tq_ready) {
        HIP_TRY(hipStreamSynchronize(s));
        if (job->stream2) HIP_TRY(hipStreamSynchronize(job->stream2));
        STEP(viterbi_transitions(job, s, err, errlen));
        job->vit_tq_ready = true;
    }
    HIP_TRY(hipEventRecord(job->ev_vit[0], s));
    pgk_launch_viterbi(job->d_contigs, (uint32_t)job->chains.size(), job->max_v, job->vit_bits, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(job->ev_vit[1], s));
    return PG_OK;
}

// Both streams are idle: the kernel classes' and the Viterbi's milliseconds from their events.  Touches no stream.
int read_timings(pg_job* job, const RunPlan& plan, char* err, size_t errlen) {
    if (plan.genotype) {
        for (int i = 0; i < PG_N_KERNEL_CLASSES; ++i) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, job->ev[i], job->ev[i + 1]));
            job->ms[i] = ms;
        }
    }
    if (job->max_v > 0 && job->params.run_phasing) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, job->ev_vit[0], job->ev_vit[1]));
        job->vit_ms = ms;
    }
    return PG_OK;
}

// The device error bits, in the order a chain's bits are reported: the first row whose bit is set names the run's error.
struct DevErr { uint32_t bit; int rc; const char* fmt; int arg; };   // fmt: the chain (%u), then `arg` (%d) where the text has one
const DevErr kDevErrs[] = {
    {PG_DEVERR_ALLELE_NOT_FOUND, PG_ERR_INVALID, "chain %u: a path_allele value is not in the variant's allele list", 0},
    {PG_DEVERR_TOO_MANY_ALLELES, PG_ERR_UNSUPPORTED, "chain %u: a variant has more than %d alleles (device limit)", PG_MAX_ALLELES_PER_VARIANT},
    {PG_DEVERR_SYNC_TIMEOUT, PG_ERR_DEVICE, "chain %u: the persistent phase-2 kernels lost each other (a chunk flag did not arrive within 10 s); without PG_KERNELS=persist phase 2 takes a launch per chunk", 0},
    {PG_DEVERR_WIDE_FUSED, PG_ERR_UNSUPPORTED, "chain %u: its only column carries more than %d alleles on the selected paths, which a fused job cannot genotype (PG_SWEEP_MODE=chunked)", PG_AMAX},
    {PG_DEVERR_TOO_MANY_LOCAL, PG_ERR_UNSUPPORTED, "chain %u: a column has more than %d distinct alleles on the selected paths (device limit)", PG_WIDE_MAX},
};

// Column counts and error bits come back; the run counts as made (job->ran, host_s[2]) before the first chain with an error bit
// ends it — the chains behind that one keep the column counts of the run before.  Touches no stream (blocking copies).
int read_errors(pg_job* job, double t_run, char* err, size_t errlen) {
    const uint32_t n = (uint32_t)job->chains.size();
    std::vector<uint32_t> ncols(n), errs(n);
    {   // (column counts and the index-level kernels' error bits are per index contig)
        const size_t ni = job->index.size();
        std::vector<uint32_t> nc_ix(ni), err_ix(ni);
        HIP_TRY(hipMemcpy(nc_ix.data(), job->d_ncols, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(err_ix.data(), job->d_ixerr, sizeof(uint32_t) * ni, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(errs.data(), job->d_err, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) { ncols[i] = nc_ix[job->chains[i].index]; errs[i] |= err_ix[job->chains[i].index]; }
    }
    job->ran = true;
    ++job->run_serial;
    job->host_s[2] = now_s() - t_run;
    for (uint32_t i = 0; i < n; ++i) {
        job->chains[i].n_cols_host = ncols[i];
        for (const DevErr& e : kDevErrs)
            if (errs[i] & e.bit) { set_err(err, errlen, e.fmt, i, e.arg); return e.rc; }
    }
    return PG_OK;
}

}  // namespace

extern "C" int pg_job_run(pg_job* job, void* stream_, char* err, size_t errlen) {
    if (!job) { set_err(err, errlen, "null job"); return PG_ERR_INVALID; }
    const double t_run = now_s();
    HIP_TRY(hipSetDevice(job->device));
    hipStream_t s = stream_ ? (hipStream_t)stream_ : job->stream;
    job->host_s[3] = 0.0;
    RunPlan plan;
    plan.genotype = job->max_v > 0 && job->params.run_genotyping;
    STEP(settle_late_for_callers_stream(job, s, &plan, err, errlen));
    plan.persist_now = job->persist && plan.genotype && streams_concurrent(job, s);   // (may replace stream2)
    if (job->persist && plan.genotype) (plan.persist_now ? job->persist_runs : job->persist_fallbacks) += 1;
    // (the preparation in parts goes with phase 1 in pieces on the job's own stream; the pipelined first run and a caller's stream
    //  keep the whole preparation ahead)
    plan.prep_beside_now = plan.genotype && job->prep_beside && s == job->stream && !job->late_pending;
    if (plan.prep_beside_now) STEP(prep_part_extents(job, err, errlen));
    HIP_TRY(hipMemsetAsync(job->zero_base, 0, job->zero_bytes, s));
    if (plan.genotype) {
        HIP_TRY(hipEventRecord(job->ev[0], s));
        if (job->late_pending) {
            STEP(first_run_pipelined(job, s, err, errlen));
        } else {
            if (plan.prep_beside_now) STEP(prepare_in_parts(job, s, err, errlen));
            else STEP(prepare(job, s, plan.index_b_due, err, errlen));
            STEP(phase1(job, s, &plan, err, errlen));
        }
        if (!job->chunked) STEP(phase2_fused(job, s, err, errlen));
        else if (plan.persist_now) STEP(phase2_persistent(job, s, err, errlen));
        else if (job->sparse2) STEP(phase2_sparse(job, s, plan, err, errlen));
        else STEP(phase2_chunks(job, s, err, errlen));
    } else if (job->max_v > 0) {
        STEP(records_only(job, s, err, errlen));
    }
    if (job->max_v > 0 && job->params.run_phasing) STEP(phase_viterbi(job, s, err, errlen));
    HIP_TRY(hipStreamSynchronize(s));
    if (job->stream2) HIP_TRY(hipStreamSynchronize(job->stream2));
    STEP(read_timings(job, plan, err, errlen));
    return read_errors(job, t_run, err, errlen);
}
