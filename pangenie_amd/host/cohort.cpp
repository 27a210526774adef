// cohort.cpp — the job drivers declared in pangenie_host.hpp, graph_io.hpp and kmer_counts.hpp: run_contigs_multi_gpu and every
// genotype_cohort* / genotype_subsets* function.  What they share — the index view of the chromosomes, the samples' rows, the
// owners of the device objects, the fetch of a chain's bins, the calls the device leaves to the host — is written once, up front.
#include "pangenie_host.hpp"
#include "kmer_counts.hpp"
#include "graph_io.hpp"
#include "host_errors.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace pangenie {

namespace {

// ------------------------------------------------------------------ owners of the device objects
// a job, or a batch's counts on the device, goes with its owner: whatever is thrown once it exists, its device memory is freed
struct JobDelete { void operator()(pg_job* job) const { pg_job_destroy(job); } };
struct CountsDelete { void operator()(pg_sampler_counts* counts) const { pg_sampler_counts_destroy(counts); } };
using Job = std::unique_ptr<pg_job, JobDelete>;
using SamplerCounts = std::unique_ptr<pg_sampler_counts, CountsDelete>;

pg_hmm_params genotyping_params(double recombrate, bool uniform, long double effective_N) {
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    return prm;
}

// ------------------------------------------------------------------ results of one chain of a job
// vector<GenotypingResult> of one chain from its packed posteriors (reference src/hmm.cpp:364-368, 106-109); kept columns
// and allele presence by the ColumnIndexer rule on the host (src/columnindexer.cpp:24-31).  `coverage` = the chain's own
// local coverages (a cohort's chains share the index, not these).
std::vector<GenotypingResult> results_of_chain(const FlatContig& f, const uint16_t* coverage, const std::vector<uint64_t>& goff,
                                               const double* lik, const int32_t* lexp) {
    const size_t V = f.variant_pos.size(), H = f.paths.size();
    std::vector<GenotypingResult> out(V);
    size_t columns = 0;
    std::vector<uint8_t> kept(V, 0), present(f.allele_id.size(), 0);
    for (size_t v = 0; v < V; ++v) {
        const uint32_t a0 = f.allele_off[v], A = f.allele_off[v + 1] - a0;
        for (size_t p = 0; p < H; ++p) {
            const uint16_t a = f.path_allele[v * H + p];
            for (uint32_t q = 0; q < A; ++q)
                if (f.allele_id[a0 + q] == a) { present[a0 + q] = 1; if (a != 0 && !(f.allele_flags[a0 + q] & 1)) kept[v] = 1; }
        }
        columns += kept[v];
    }
    for (size_t v = 0; v < V; ++v) {
        GenotypingResult& g = out[v];
        if (kept[v]) {
            const uint32_t a0 = f.allele_off[v], A = f.allele_off[v + 1] - a0;
            for (uint32_t a = 0; a < A; ++a) {
                if (!present[a0 + a]) continue;
                for (uint32_t b = a; b < A; ++b) {
                    if (!present[a0 + b]) continue;
                    const uint64_t idx = goff[v] + (uint64_t)a * A - (uint64_t)a * (a - 1) / 2 + (b - a);
                    g.add_to_likelihood(f.allele_id[a0 + a], f.allele_id[a0 + b], ldexpl((long double)lik[idx], lexp[idx]));
                }
            }
        }
        if (columns > 0) {  // reference src/hmm.cpp:94,106-109
            g.set_unique_kmers((unsigned short)(f.kmer_off[v + 1] - f.kmer_off[v]));
            g.set_coverage(coverage[v]);
        }
    }
    return out;
}

// One chain's bins from the device as one GenotypingResult per variant.  `coverage` = the chain's local coverages, or null: then
// they are what pg_job_fetch hands out (a chain whose counts never were on the host).  pg_job_fetch hands the coverage out only
// when the chain has columns: exactly when results_of_chain reads it.  Returns the C ABI's code, its text in `err`.
int fetch_chain_results(pg_job* job, uint32_t chain, const FlatContig& f, const std::vector<uint64_t>& goff, const uint16_t* coverage,
                        std::vector<GenotypingResult>* results, char* err, size_t errlen) {
    const uint64_t n = goff.back();
    const size_t V = f.variant_pos.size();
    std::vector<double> lik(n ? n : 1);
    std::vector<int32_t> lexp(n ? n : 1);
    std::vector<uint16_t> cov(coverage ? 0 : V ? V : 1);
    pg_contig_result res{};
    res.lik = lik.data(); res.lik_exp = lexp.data();
    if (!coverage) res.coverage = cov.data();
    const int rc = pg_job_fetch(job, chain, &res, err, errlen);
    if (rc == PG_OK) *results = results_of_chain(f, coverage ? coverage : cov.data(), goff, lik.data(), lexp.data());
    return rc;
}

// Per variant of one chain its k-mer count and coverage by pg_job_fetch's rule (a chain without a kept column reports neither,
// `n_columns` = 0): host memory of the job, no device copy.  Returns the C ABI's code, its text in `err`.
int fetch_chain_meta(pg_job* job, uint32_t chain, size_t V, std::vector<uint16_t>* n_kmers, std::vector<uint16_t>* coverage, uint32_t* n_columns,
                     char* err, size_t errlen) {
    n_kmers->assign(V ? V : 1, 0);
    coverage->assign(V ? V : 1, 0);
    pg_contig_result meta{};
    meta.n_kmers = n_kmers->data(); meta.coverage = coverage->data();
    const int rc = pg_job_fetch(job, chain, &meta, err, errlen);
    n_kmers->resize(V);
    coverage->resize(V);
    if (n_columns) *n_columns = meta.n_columns;
    return rc;
}

// ------------------------------------------------------------------ the index and the samples as a cohort job takes them
// What the drivers need of one chromosome: depends on the index alone, made once whatever the samples and batches.
struct Chromosome {
    std::string name;
    FlatContig flat;              // ALL paths of the panel (the phasing drivers: the selected ones)
    std::vector<uint64_t> goff;   // pg_hmm_geno_offsets of `flat`
    // what the functions that return VCF records add (add_record_plans, record_chromosomes)
    const Graph* graph = nullptr;
    RecordPlan plan;
    std::vector<uint64_t> gl_off;
    bool host_route = false;      // the phasing drivers: no plan on the device, the column is formed here (phase_cohort_record_text)
};

// the index view of `chromosomes` over all paths (or `only_paths`), in the order of the map (a DeviceCountPlan's too)
std::vector<Chromosome> index_chromosomes(std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes,
                                          std::vector<unsigned short>* only_paths = nullptr) {
    std::vector<Chromosome> chroms(chromosomes.size());
    size_t c = 0;
    for (auto& kv : chromosomes) {
        Chromosome& x = chroms[c++];
        x.name = kv.first;
        flatten(&kv.second, only_paths, x.flat);
        x.goff.assign(x.flat.variant_pos.size() + 1, 0);
        pg_hmm_geno_offsets(&x.flat.batch, x.goff.data());
    }
    return chroms;
}

std::vector<pg_contig_batch> batches_of(const std::vector<Chromosome>& chroms) {
    std::vector<pg_contig_batch> batches;
    for (const Chromosome& x : chroms) batches.push_back(x.flat.batch);
    return batches;
}

// refuses a missing graph or one whose bubble count is not the index's; needs no device
const Graph& graph_of(const std::map<std::string, Graph>& graphs, const std::string& name, size_t bubbles, const char* who) {
    const auto g = graphs.find(name);
    if (g == graphs.end() || g->second.size() != bubbles) fail(std::string(who) + ": no graph of " + name + " with the index's bubbles");
    return g->second;
}

void add_record_plans(std::vector<Chromosome>& chroms, const std::map<std::string, Graph>& graphs, const char* who) {
    for (Chromosome& x : chroms) {
        x.graph = &graph_of(graphs, x.name, x.flat.variant_pos.size(), who);
        x.plan = x.graph->record_plan();
    }
}

// the offsets of a plan's GL values: they hang on the plan alone
std::vector<uint64_t> record_gl_offsets(const RecordPlan& plan, const std::string& refusal) {
    std::vector<uint64_t> gl_off(plan.nr_of_records() + 1, 0);
    const pg_record_plan view = plan.view();
    if (pg_record_gl_offsets(&view, gl_off.data()) != PG_OK) fail(refusal);
    return gl_off;
}

// the index with all that the record tail of a sampled cohort needs of it
std::vector<Chromosome> record_chromosomes(std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes,
                                           const std::map<std::string, Graph>& graphs, const char* who) {
    std::vector<Chromosome> chroms = index_chromosomes(chromosomes);
    add_record_plans(chroms, graphs, who);
    for (Chromosome& x : chroms) x.gl_off = record_gl_offsets(x.plan, std::string(who) + ": pg_record_gl_offsets refused the record plan of " + x.name);
    return chroms;
}

// per sample the two pointer rows of pg_sample_counts; sizes checked against the index (`who`: the caller's name in the refusal)
struct SampleRows {
    std::vector<std::vector<const uint16_t*>> count_rows, cov_rows;   // [S][C]
    std::vector<pg_sample_counts> rows;                                // [S], into the two above
};

SampleRows sample_rows(const std::vector<SampleCounts>& samples, const std::vector<Chromosome>& chroms, const char* who) {
    static const uint16_t none = 0;
    const size_t S = samples.size(), C = chroms.size();
    SampleRows r;
    r.count_rows.assign(S, std::vector<const uint16_t*>(C));
    r.cov_rows.assign(S, std::vector<const uint16_t*>(C));
    r.rows.resize(S);
    for (size_t s = 0; s < S; ++s) {
        for (size_t c = 0; c < C; ++c) {
            const FlatContig& f = chroms[c].flat;
            const auto k = samples[s].kmer_count.find(chroms[c].name), v = samples[s].coverage.find(chroms[c].name);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != f.kmer_count.size() ||
                v->second.size() != f.variant_pos.size())
                fail(std::string(who) + ": sample " + std::to_string(s) + " does not fit the index on " + chroms[c].name);
            r.count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            r.cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        r.rows[s].kmer_count = r.count_rows[s].data();
        r.rows[s].coverage = r.cov_rows[s].data();
    }
    return r;
}

// a cohort job over the index, made and not yet run: chain id = sample * n_contigs + contig
Job cohort_job(int device, const std::vector<Chromosome>& chroms, const std::vector<pg_sample_counts>& rows, ProbabilityTable* probabilities,
               const pg_hmm_params& prm) {
    const std::vector<pg_contig_batch> index = batches_of(chroms);
    char err[512] = {0};
    pg_job* made = nullptr;
    const int rc = pg_cohort_new(device, (uint32_t)index.size(), index.data(), (uint32_t)rows.size(), rows.data(), probabilities->handle(), &prm, &made,
                                 err, sizeof(err));
    Job job(made);
    check_rc(rc, err);
    return job;
}

// ------------------------------------------------------------------ calls the device leaves to the host
GenotypeCall call_of(const pg_call& r) {
    GenotypeCall call;
    call.allele_1 = r.allele_1; call.allele_2 = r.allele_2; call.quality = r.gq;
    return call;
}

// GT and GQ of a call the device deferred — a likelihood next to long double's subnormals — from its NORMALISED likelihoods
GenotypeCall deferred_call(const GenotypingResult& normalised) {
    GenotypeCall call;
    call.deferred = true;
    const std::pair<int, int> g = normalised.get_likeliest_genotype();
    if (g.first >= 0 && g.second >= 0) {
        call.allele_1 = g.first; call.allele_2 = g.second;
        call.quality = normalised.get_genotype_quality((unsigned short)g.first, (unsigned short)g.second);
    }
    return call;
}

// One chain's calls from the device's records, one per variant: the calls are taken over, and the deferred variants are formed
// on the host, each from its own bins, through GenotypingResult.  `bins()` fetches the chain's bins as one GenotypingResult per
// variant: it is called only for a chain with a deferred variant, so no other chain's bins leave the device.
template <class Bins>
std::vector<GenotypeCall> calls_of_chain(const std::vector<pg_call>& r, Bins bins) {
    std::vector<GenotypeCall> calls(r.size());
    bool any_deferred = false;
    for (size_t v = 0; v < r.size(); ++v) {
        if (r[v].flags == PG_CALL_OK) calls[v] = call_of(r[v]);
        else if (r[v].flags == PG_CALL_DEFERRED) any_deferred = true;
    }
    if (!any_deferred) return calls;
    std::vector<GenotypingResult> full = bins();
    for (size_t v = 0; v < r.size(); ++v) {
        if (r[v].flags != PG_CALL_DEFERRED) continue;
        full[v].normalize();
        calls[v] = deferred_call(full[v]);
    }
    return calls;
}

}  // namespace

// ------------------------------------------------------------------ multi-GPU job loop
std::vector<std::vector<GenotypingResult>> run_contigs_multi_gpu(std::vector<ContigTask>& tasks, ProbabilityTable* probabilities,
                                                                 double recombrate, bool uniform, long double effective_N,
                                                                 const std::vector<int>& devices) {
    if (devices.empty()) fail("run_contigs_multi_gpu: no devices");
    const size_t T = tasks.size(), D = devices.size();
    std::vector<FlatContig> flat(T);
    std::vector<std::vector<uint64_t>> goff(T);
    std::vector<double> weight(T);
    for (size_t t = 0; t < T; ++t) {
        flatten(tasks[t].unique_kmers, tasks[t].only_paths, flat[t]);
        const size_t V = flat[t].variant_pos.size();
        goff[t].assign(V + 1, 0);
        pg_hmm_geno_offsets(&flat[t].batch, goff[t].data());
        weight[t] = (double)V * (double)flat[t].paths.size() * (double)flat[t].paths.size();
    }
    // longest processing time first; ties by index: every host computes the same plan
    std::vector<size_t> order(T);
    for (size_t t = 0; t < T; ++t) order[t] = t;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weight[a] > weight[b]; });
    std::vector<std::vector<size_t>> plan(D);
    std::vector<double> load(D, 0.0);
    for (size_t t : order) {
        size_t best = 0;
        for (size_t d = 1; d < D; ++d) if (load[d] < load[best]) best = d;
        plan[best].push_back(t);
        load[best] += weight[t];
    }
    for (auto& p : plan) std::sort(p.begin(), p.end());

    const pg_hmm_params prm = genotyping_params(recombrate, uniform, effective_N);
    std::vector<Job> jobs(D);
    std::vector<std::string> errors(D);
    std::vector<std::thread> threads;
    for (size_t d = 0; d < D; ++d)
        threads.emplace_back([&, d] {
            if (plan[d].empty()) return;
            std::vector<pg_contig_batch> b;
            for (size_t t : plan[d]) b.push_back(flat[t].batch);
            char err[512] = {0};
            pg_job* made = nullptr;
            int rc = pg_job_new(devices[d], (uint32_t)b.size(), b.data(), probabilities->handle(), &prm, &made, err, sizeof(err));
            jobs[d].reset(made);
            if (rc == PG_OK) rc = pg_job_run(made, nullptr, err, sizeof(err));
            if (rc != PG_OK) errors[d] = err[0] ? err : "pangenie_hmm error";
        });
    for (auto& th : threads) th.join();
    for (size_t d = 0; d < D; ++d)
        if (!errors[d].empty()) fail(errors[d]);

    // ONE exchange: every device's packed posteriors to devices[0], then to the host
    std::vector<uint64_t> n_lik(D, 0);
    uint64_t total = 0;
    for (size_t d = 0; d < D; ++d) { for (size_t t : plan[d]) n_lik[d] += goff[t].back(); total += n_lik[d]; }
    std::vector<double> lik(total ? total : 1);
    std::vector<int32_t> lexp(total ? total : 1);
    char err[512] = {0};
    if (D == 1) {
        uint64_t off = 0;
        for (size_t k = 0; k < plan[0].size(); ++k) {
            pg_contig_result r{};
            r.lik = lik.data() + off; r.lik_exp = lexp.data() + off;
            check_rc(pg_job_fetch(jobs[0].get(), (uint32_t)k, &r, err, sizeof(err)), err);
            off += goff[plan[0][k]].back();
        }
    } else {
        std::vector<pg_job*> handles(D, nullptr);
        for (size_t d = 0; d < D; ++d) handles[d] = jobs[d].get();
        std::vector<pg_comm*> comms(D, nullptr);
        int rc = pg_comm_init_all((int)D, devices.data(), comms.data(), err, sizeof(err));
        if (rc == PG_OK) rc = pg_hmm_gather_to_host((int)D, comms.data(), handles.data(), 0, n_lik.data(), lik.data(), lexp.data(), err, sizeof(err));
        for (pg_comm* c : comms) if (c) pg_comm_destroy(c);
        check_rc(rc, err);
    }
    jobs.clear();   // (the device memory goes before the results are rebuilt)

    // rebuild the GenotypingResults
    std::vector<std::vector<GenotypingResult>> out(T);
    uint64_t base = 0;
    for (size_t d = 0; d < D; ++d)
        for (size_t t : plan[d]) {
            out[t] = results_of_chain(flat[t], flat[t].coverage.data(), goff[t], lik.data() + base, lexp.data() + base);
            base += goff[t].back();
        }
    return out;
}

// ------------------------------------------------------------------ cohort job
SampleCounts SampleCounts::of(const std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes) {
    SampleCounts s;
    for (const auto& kv : chromosomes) {
        std::vector<uint16_t>& counts = s.kmer_count[kv.first];
        std::vector<uint16_t>& cov = s.coverage[kv.first];
        for (const std::shared_ptr<UniqueKmers>& u : kv.second) {
            for (size_t i = 0; i < u->size(); ++i) counts.push_back(u->get_readcount_of(i));
            cov.push_back(u->get_coverage());
        }
    }
    return s;
}

std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<SampleCounts>& samples,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (C == 0 || S == 0) return out;
    const std::vector<Chromosome> chroms = index_chromosomes(chromosomes);
    const SampleRows rows = sample_rows(samples, chroms, "genotype_cohort");
    const Job job = cohort_job(device, chroms, rows.rows, probabilities, genotyping_params(recombrate, uniform, effective_N));
    char err[512] = {0};
    check_rc(pg_job_run(job.get(), nullptr, err, sizeof(err)), err);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < C; ++c)
            check_rc(fetch_chain_results(job.get(), (uint32_t)(s * C + c), chroms[c].flat, chroms[c].goff, rows.cov_rows[s][c], &out[s][chroms[c].name], err,
                                         sizeof(err)),
                     err);
    return out;
}

// ------------------------------------------------------------------ cohort job, calls instead of likelihoods
std::vector<std::map<std::string, std::vector<GenotypeCall>>> genotype_cohort_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<SampleCounts>& samples,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, std::vector<GenotypeCall>>> out(S);
    if (C == 0 || S == 0) return out;
    const std::vector<Chromosome> chroms = index_chromosomes(chromosomes);
    const SampleRows rows = sample_rows(samples, chroms, "genotype_cohort_calls");
    const Job job = cohort_job(device, chroms, rows.rows, probabilities, genotyping_params(recombrate, uniform, effective_N));
    char err[512] = {0};
    int rc = pg_job_run(job.get(), nullptr, err, sizeof(err));
    if (rc == PG_OK) rc = pg_job_calls(job.get(), err, sizeof(err));
    check_rc(rc, err);
    // all records with one synchronisation
    std::vector<std::vector<pg_call>> recs(S * C);
    std::vector<pg_call*> ptrs(S * C, nullptr);
    for (size_t i = 0; i < S * C; ++i) {
        recs[i].resize(chroms[i % C].flat.variant_pos.size());
        ptrs[i] = recs[i].empty() ? nullptr : recs[i].data();
    }
    check_rc(pg_job_fetch_calls_all(job.get(), ptrs.data(), err, sizeof(err)), err);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < C; ++c)
            out[s][chroms[c].name] = calls_of_chain(recs[s * C + c], [&] {
                std::vector<GenotypingResult> full;
                check_rc(fetch_chain_results(job.get(), (uint32_t)(s * C + c), chroms[c].flat, chroms[c].goff, rows.cov_rows[s][c], &full, err, sizeof(err)), err);
                return full;
            });
    return out;
}

// ------------------------------------------------------------------ path subsets: one job, combined on the device
namespace {

// The -a flow as ONE job: chain c * S + s = chromosome c over subsets[s]; group c = its S chains in the order of `subsets`.
struct SubsetsRun {
    size_t C = 0, S = 0;
    std::vector<std::string> names;
    std::vector<FlatContig> flat;              // [C * S]
    std::vector<std::vector<uint64_t>> goff;   // [C]
    Job job;
    char err[512] = {0};

    void run(std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<std::vector<unsigned short>>& subsets,
             ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
        C = chromosomes.size(); S = subsets.size();
        flat.resize(C * S);
        goff.resize(C);
        std::vector<pg_contig_batch> batches(C * S);
        std::vector<uint32_t> group_off(C + 1, 0), chains(C * S);
        size_t c = 0;
        for (auto& kv : chromosomes) {
            names.push_back(kv.first);
            for (size_t s = 0; s < S; ++s) {
                std::vector<unsigned short> paths = subsets[s];
                flatten(&kv.second, &paths, flat[c * S + s]);
                batches[c * S + s] = flat[c * S + s].batch;
                chains[c * S + s] = (uint32_t)(c * S + s);
            }
            goff[c].assign(flat[c * S].variant_pos.size() + 1, 0);
            pg_hmm_geno_offsets(&flat[c * S].batch, goff[c].data());
            group_off[c + 1] = (uint32_t)((c + 1) * S);
            c += 1;
        }
        const pg_hmm_params prm = genotyping_params(recombrate, uniform, effective_N);
        pg_job* made = nullptr;
        int rc = pg_job_new(device, (uint32_t)(C * S), batches.data(), probabilities->handle(), &prm, &made, err, sizeof(err));
        job.reset(made);
        if (rc == PG_OK) rc = pg_job_run(made, nullptr, err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_combine_plan(made, (uint32_t)C, group_off.data(), chains.data(), err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_combine(made, err, sizeof(err));
        check_rc(rc, err);
    }

    // chromosome c on the host route: every subset's chain from its fetched bins, combine_likelihoods in the order of the subsets
    std::vector<GenotypingResult> combined_on_host(size_t c) {
        std::vector<GenotypingResult> total;
        for (size_t s = 0; s < S; ++s) {
            const FlatContig& f = flat[c * S + s];
            static const uint16_t none = 0;
            std::vector<GenotypingResult> one;
            check_rc(fetch_chain_results(job.get(), (uint32_t)(c * S + s), f, goff[c], f.coverage.empty() ? &none : f.coverage.data(), &one, err, sizeof(err)), err);
            if (s == 0) total = std::move(one);
            else for (size_t v = 0; v < total.size(); ++v) total[v].combine(one[v]);
        }
        return total;
    }

    // unique_kmers and coverage of chromosome c are those of its first chain (GenotypingResult::combine leaves them alone)
    void first_chain_meta(size_t c, std::vector<uint16_t>* n_kmers, std::vector<uint16_t>* cov) {
        check_rc(fetch_chain_meta(job.get(), (uint32_t)(c * S), flat[c * S].variant_pos.size(), n_kmers, cov, nullptr, err, sizeof(err)), err);
    }
};

}  // namespace

std::map<std::string, std::vector<GenotypingResult>> genotype_subsets(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<std::vector<unsigned short>>& subsets,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool normalize) {
    std::map<std::string, std::vector<GenotypingResult>> out;
    if (subsets.empty()) fail("genotype_subsets: no subsets of paths");
    if (chromosomes.empty()) return out;
    SubsetsRun R;
    R.run(chromosomes, subsets, probabilities, recombrate, uniform, effective_N, device);
    const size_t C = R.C, S = R.S;
    // all combined bins with one synchronisation
    std::vector<std::vector<pg_combined_bin>> bins(C);
    std::vector<pg_combined_bin*> ptrs(C, nullptr);
    for (size_t c = 0; c < C; ++c) {
        bins[c].resize(R.goff[c].back());
        ptrs[c] = bins[c].empty() ? nullptr : bins[c].data();
    }
    check_rc(pg_job_fetch_combined_all(R.job.get(), ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) {
        const FlatContig& f = R.flat[c * S];
        const size_t V = f.variant_pos.size();
        std::vector<GenotypingResult>& res = out[R.names[c]];
        res.resize(V);
        std::vector<uint16_t> n_kmers, cov;
        R.first_chain_meta(c, &n_kmers, &cov);
        std::vector<size_t> deferred;
        for (size_t v = 0; v < V; ++v) {
            GenotypingResult& g = res[v];
            const uint32_t a0 = f.allele_off[v], A = f.allele_off[v + 1] - a0;
            const pg_combined_bin* b = bins[c].data() + R.goff[c][v];
            bool any_deferred = false;
            for (uint32_t x = 0; x < A; ++x)
                for (uint32_t y = x; y < A; ++y, ++b) {
                    if (!(b->flags & PG_COMBINED_PRESENT)) continue;
                    if (b->flags & PG_COMBINED_DEFERRED) { any_deferred = true; continue; }
                    g.add_to_likelihood(f.allele_id[a0 + x], f.allele_id[a0 + y], ldexpl((long double)b->m, b->e));   // exact
                }
            g.set_unique_kmers(n_kmers[v]);
            g.set_coverage(cov[v]);
            if (any_deferred) deferred.push_back(v);
        }
        if (!deferred.empty()) {   // keys next to long double's subnormals: those variants from the chains' own bins
            std::vector<GenotypingResult> full = R.combined_on_host(c);
            for (size_t v : deferred) {
                full[v].set_unique_kmers(n_kmers[v]);
                full[v].set_coverage(cov[v]);
                res[v] = full[v];
            }
        }
        if (normalize) for (GenotypingResult& g : res) g.normalize();
    }
    return out;
}

std::map<std::string, std::vector<GenotypeCall>> genotype_subsets_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<std::vector<unsigned short>>& subsets,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    std::map<std::string, std::vector<GenotypeCall>> out;
    if (subsets.empty()) fail("genotype_subsets_calls: no subsets of paths");
    if (chromosomes.empty()) return out;
    SubsetsRun R;
    R.run(chromosomes, subsets, probabilities, recombrate, uniform, effective_N, device);
    check_rc(pg_job_combined_calls(R.job.get(), R.err, sizeof(R.err)), R.err);
    const size_t C = R.C, S = R.S;
    std::vector<std::vector<pg_call>> recs(C);
    std::vector<pg_call*> ptrs(C, nullptr);
    for (size_t c = 0; c < C; ++c) {
        recs[c].resize(R.flat[c * S].variant_pos.size());
        ptrs[c] = recs[c].empty() ? nullptr : recs[c].data();
    }
    check_rc(pg_job_fetch_combined_calls_all(R.job.get(), ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) out[R.names[c]] = calls_of_chain(recs[c], [&] { return R.combined_on_host(c); });
    return out;
}

// ------------------------------------------------------------------ calls and GL values per VCF record
namespace {

// this site's likelihoods restricted to its defined alleles, as genotype_field takes them (graph.cpp:225-233); `n_defined`: how many
GenotypingResult defined_likelihoods(const VcfSite& site, size_t* n_defined = nullptr) {
    GenotypingResult tmp = site.likelihoods;
    if (tmp.contains_no_likelihoods()) tmp.add_to_likelihood(0, 0, 1.0);
    std::vector<unsigned short> defined = {0};
    for (size_t a = 1; a < site.alleles.size(); ++a)
        if (!site.undefined[a]) defined.push_back((unsigned short)a);
    if (n_defined) *n_defined = defined.size();
    return defined.size() < site.alleles.size() ? tmp.get_specific_likelihoods(defined) : tmp;
}

// GT and GQ of one record as genotype_field prints them (graph.cpp:217-273), without the text
GenotypeCall record_call_on_host(const VcfSite& site) {
    return deferred_call(defined_likelihoods(site));
}

// the four digits of a long double logarithm as the device stores them: glibc prints the exact decimal expansion
pg_gl gl_of_log10(long double v) {
    pg_gl g;
    g.mant = 0;
    if (std::isinf(v) || std::isnan(v)) { g.exp10 = PG_GL_NEG_INF; return g; }   // (log10 of 0; a likelihood is never negative)
    if (v == 0.0L) { g.exp10 = 0; return g; }
    char buf[48];
    std::snprintf(buf, sizeof(buf), "%.3Le", v);   // [-]d.ddde[+-]XX
    const char* p = buf;
    const bool negative = *p == '-';
    if (negative) ++p;
    const int mant = (p[0] - '0') * 1000 + (p[2] - '0') * 100 + (p[3] - '0') * 10 + (p[4] - '0');
    g.mant = (int16_t)(negative ? -mant : mant);
    g.exp10 = (int16_t)std::atoi(p + 6);
    return g;
}

// the GL values of one record as genotype_field prints them, from the bubble's bins on the host
void record_gl_on_host(const VcfSite& site, pg_gl* out, size_t n) {
    size_t n_defined = 0;
    const GenotypingResult gl = defined_likelihoods(site, &n_defined);
    const std::vector<long double> all = gl.get_all_likelihoods(n_defined);
    if (all.size() != n) fail("genotype_cohort_record_fields: a record's likelihoods do not fit its GL values");
    for (size_t j = 0; j < n; ++j) out[j] = gl_of_log10(std::log10(all[j]));
}

// One chain's record fields from the device's records `r` (one per record of `plan`; with `with_gl`, fields.gl and
// fields.gl_off hold the chain's values already): the calls are taken over, and what the device deferred — a bubble next to
// long double's subnormals, a GL value in the 1e-9 window — is finished here from that chain's own bins through
// Variant::records and genotype_field's rules.  The tail of every function that returns RecordFields.  `no_kmers(v)`: bubble
// v reports no unique k-mers; `results(&full)` fetches the chain's bins as one GenotypingResult per bubble and returns the C
// ABI's code: it is called only for a chain with a deferred entry, so no other chain's bins leave the device.
template <class NoKmers, class Results>
int chain_record_fields(const Graph& graph, const RecordPlan& plan, const pg_call* r, bool ignore_imputed, bool with_gl, NoKmers no_kmers,
                        Results results, RecordFields& fields) {
    std::vector<GenotypeCall>& calls = fields.calls;
    calls.assign(plan.nr_of_records(), GenotypeCall());
    bool any_deferred = false;
    std::vector<char> gl_deferred(with_gl ? plan.rec_off.size() - 1 : 0, 0);   // per bubble: a GL value is left to the host
    for (size_t v = 0; v < gl_deferred.size(); ++v)
        for (uint64_t i = fields.gl_off[plan.rec_off[v]]; i < fields.gl_off[plan.rec_off[v + 1]]; ++i)
            if (fields.gl[i].mant == 0 && fields.gl[i].exp10 == PG_GL_DEFERRED) { gl_deferred[v] = 1; any_deferred = true; }
    for (size_t v = 0; v + 1 < plan.rec_off.size(); ++v) {
        const bool imputed = ignore_imputed && no_kmers(v);
        for (size_t q = plan.rec_off[v]; q < plan.rec_off[v + 1]; ++q) {
            if (imputed) continue;   // `.`: genotype_field drops the genotype of a bubble without unique k-mers
            if ((r[q].flags & 0xFF) == PG_CALL_OK) calls[q] = call_of(r[q]);
            else if (r[q].flags == PG_CALL_DEFERRED) any_deferred = true;
        }
    }
    if (!any_deferred) return PG_OK;
    // the deferred bubbles of this chain on the host, each from its own bins, through Variant::records
    std::vector<GenotypingResult> full;
    const int rc = results(&full);
    if (rc != PG_OK) return rc;
    for (size_t v = 0; v + 1 < plan.rec_off.size(); ++v) {
        const bool call_deferred = r[plan.rec_off[v]].flags == PG_CALL_DEFERRED;   // (a bubble is deferred with all its records)
        const bool imputed = ignore_imputed && full[v].nr_unique_kmers() == 0;
        const bool calls_here = call_deferred && !imputed, gl_here = with_gl && gl_deferred[v];
        if (!calls_here && !gl_here) continue;
        full[v].normalize();
        const std::vector<VcfSite> sites = graph.get_variant(v).records(&full[v]);
        for (size_t k = 0; k < sites.size() && plan.rec_off[v] + k < plan.rec_off[v + 1]; ++k) {
            const size_t q = plan.rec_off[v] + k;
            if (calls_here) calls[q] = record_call_on_host(sites[k]);
            if (gl_here) record_gl_on_host(sites[k], fields.gl.data() + fields.gl_off[q], fields.gl_off[q + 1] - fields.gl_off[q]);   // (the GL column is printed whatever ignore_imputed says)
        }
    }
    return PG_OK;
}

// The text of a job's sample columns to the host: pg_job_record_text, then ONE copy of the packed bytes and
// their offsets.  calls_first[n_chains + 1] = every chain's first record, off = every record's first byte in `packed`.
int job_record_text(pg_job* job, size_t n_chains, bool ignore_imputed, std::vector<uint64_t>* calls_first, std::vector<uint64_t>* off,
                    std::string* packed, char* err, size_t errlen) {
    int rc = pg_job_record_text(job, ignore_imputed ? 1 : 0, err, errlen);
    std::vector<uint64_t> text_first(n_chains + 1, 0);
    calls_first->assign(n_chains + 1, 0);
    if (rc == PG_OK) rc = pg_job_record_text_first(job, text_first.data(), err, errlen);
    if (rc == PG_OK) rc = pg_job_record_first(job, calls_first->data(), nullptr, err, errlen);
    if (rc != PG_OK) return rc;
    off->assign(calls_first->back() + 1, 0);
    packed->assign(text_first.back(), '\0');
    return pg_job_fetch_record_text_packed(job, off->data(), packed->empty() ? nullptr : &(*packed)[0], packed->size(), err, errlen);
}

// One chain's RecordText from the packed text (`off`: the chain's R + 1 absolute offsets).  A record the device left to the host
// — empty although it has three values or more: a deferred call or GL value — is finished as chain_record_fields finishes it,
// from this chain's fetched calls and GL values and, through `results`, its bins, and printed by record_field_text;
// `coverage(v)`: KC of bubble v.  No other chain's fields leave the device.
template <class NoKmers, class Coverage, class Results>
int chain_record_text(pg_job* job, uint32_t chain, const Chromosome& x, bool ignore_imputed, const uint64_t* off, const std::string& packed,
                      NoKmers no_kmers, Coverage coverage, Results results, RecordText& out, char* err, size_t errlen) {
    const RecordPlan& plan = x.plan;
    const size_t R = plan.nr_of_records();
    out.off.assign(R + 1, 0);
    for (size_t q = 0; q <= R; ++q) out.off[q] = off[q] - off[0];
    out.bytes.assign(packed, off[0], off[R] - off[0]);
    std::vector<size_t> pending;
    for (size_t q = 0; q < R; ++q)
        if (out.off[q + 1] == out.off[q] && x.gl_off[q + 1] - x.gl_off[q] >= 3) pending.push_back(q);
    if (pending.empty()) return PG_OK;
    RecordFields fields;
    fields.gl_off = x.gl_off;
    fields.gl.resize(x.gl_off.back());
    std::vector<pg_call> r(R);
    int rc = pg_job_fetch_record_calls(job, chain, r.data(), err, errlen);
    if (rc == PG_OK) rc = pg_job_fetch_record_gl(job, chain, fields.gl.data(), err, errlen);
    if (rc == PG_OK) rc = chain_record_fields(*x.graph, plan, r.data(), ignore_imputed, true, no_kmers, results, fields);
    if (rc != PG_OK) return rc;
    std::vector<size_t> bubble(R, 0);
    for (size_t v = 0; v + 1 < plan.rec_off.size(); ++v)
        for (size_t q = plan.rec_off[v]; q < plan.rec_off[v + 1]; ++q) bubble[q] = v;
    std::string bytes;
    std::vector<uint64_t> spliced(R + 1, 0);
    size_t p = 0;
    for (size_t q = 0; q < R; ++q) {
        spliced[q] = bytes.size();
        if (p < pending.size() && pending[p] == q) {
            bytes += record_field_text(fields, q, coverage(bubble[q]), ignore_imputed && no_kmers(bubble[q]));
            ++p;
        } else bytes.append(out.bytes, out.off[q], out.off[q + 1] - out.off[q]);
    }
    spliced[R] = bytes.size();
    out.off.swap(spliced);
    out.bytes.swap(bytes);
    return PG_OK;
}

// ------------------------------------------------------------------ cohort job, the sample column per VCF record
using CoverageRows = std::vector<std::vector<const uint16_t*>>;   // [sample][chromosome], SampleRows::cov_rows

// The job of the genotype_cohort_record_* and phase_cohort_record_* functions: a cohort job over all paths or `only_paths`
// under `prm`, with one record plan per chromosome, whatever the number of samples — none for a chromosome `on_host(graph)`
// keeps for the host route —, made and run; then `tail(job, chroms, cov_rows)`: exactly one of the tails below.  `who`: the
// name in a refusal.
template <class OnHost, class Tail>
void run_record_cohort(std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
                       const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, std::vector<unsigned short>* only_paths, const pg_hmm_params& prm,
                       int device, const char* who, OnHost on_host, Tail tail) {
    if (chromosomes.empty() || samples.empty()) return;
    std::vector<Chromosome> chroms = index_chromosomes(chromosomes, only_paths);
    add_record_plans(chroms, graphs, who);
    for (Chromosome& x : chroms) x.host_route = on_host(*x.graph);   // (every graph is looked at once)
    const SampleRows rows = sample_rows(samples, chroms, who);
    const Job job = cohort_job(device, chroms, rows.rows, probabilities, prm);
    char err[512] = {0};
    int rc = PG_OK;
    for (size_t c = 0; c < chroms.size() && rc == PG_OK; ++c) {
        if (chroms[c].host_route) continue;
        const pg_record_plan view = chroms[c].plan.view();
        rc = pg_job_record_plan(job.get(), (uint32_t)c, &view, err, sizeof(err));
    }
    if (rc == PG_OK) rc = pg_job_run(job.get(), nullptr, err, sizeof(err));
    check_rc(rc, err);
    tail(job.get(), chroms, rows.cov_rows);
}

// ... of the four genotype_cohort_record_* functions: all paths, the genotyping.  (All four name genotype_cohort_record_calls in
// a refusal: callers match on these texts.)
template <class Tail>
void run_record_cohort(std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
                       const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N,
                       int device, Tail tail) {
    run_record_cohort(chromosomes, graphs, samples, probabilities, nullptr, genotyping_params(recombrate, uniform, effective_N), device,
                      "genotype_cohort_record_calls", [](const Graph&) { return false; }, tail);
}

void add_gl_offsets(std::vector<Chromosome>& chroms) {
    for (Chromosome& x : chroms) x.gl_off = record_gl_offsets(x.plan, "pg_record_gl_offsets refused the record plan");
}

// a chain without a kept column reports no unique k-mers (results_of_chain); a sampled chain asks pg_job_fetch instead
bool any_kept_column(const FlatContig& f) {
    const size_t H = f.paths.size();
    for (size_t v = 0; v < f.variant_pos.size(); ++v)
        for (size_t p = 0; p < H; ++p) {
            const uint16_t a = f.path_allele[v * H + p];
            for (uint32_t q = f.allele_off[v]; q < f.allele_off[v + 1]; ++q)
                if (f.allele_id[q] == a && a != 0 && !(f.allele_flags[q] & 1)) return true;
        }
    return false;
}

// the calls and, `with_gl`, the GL values per record: out[s] = sample s
void cohort_record_fields(pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows, bool ignore_imputed, bool with_gl,
                          std::vector<std::map<std::string, RecordFields>>* out) {
    const size_t C = chroms.size(), S = cov_rows.size();
    char err[512] = {0};
    int rc = pg_job_record_calls(job, err, sizeof(err));
    if (rc == PG_OK && with_gl) rc = pg_job_record_gl(job, err, sizeof(err));
    check_rc(rc, err);
    if (with_gl) add_gl_offsets(chroms);
    // all records with one synchronisation
    std::vector<std::vector<pg_call>> recs(S * C);
    std::vector<pg_call*> ptrs(S * C, nullptr);
    for (size_t i = 0; i < S * C; ++i) {
        recs[i].resize(chroms[i % C].plan.nr_of_records());
        ptrs[i] = recs[i].empty() ? nullptr : recs[i].data();
    }
    check_rc(pg_job_fetch_record_calls_all(job, ptrs.data(), err, sizeof(err)), err);
    if (with_gl) {   // ... and all GL values with another
        std::vector<pg_gl*> gl_ptrs(S * C, nullptr);
        for (size_t i = 0; i < S * C; ++i) {
            RecordFields& fields = (*out)[i / C][chroms[i % C].name];
            fields.gl_off = chroms[i % C].gl_off;
            fields.gl.resize(fields.gl_off.back());
            gl_ptrs[i] = fields.gl.empty() ? nullptr : fields.gl.data();
        }
        check_rc(pg_job_fetch_record_gl_all(job, gl_ptrs.data(), err, sizeof(err)), err);
    }
    std::vector<char> any_column(C);
    for (size_t c = 0; c < C; ++c) any_column[c] = any_kept_column(chroms[c].flat);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < C; ++c) {
            const Chromosome& x = chroms[c];
            const FlatContig& f = x.flat;
            const uint32_t chain = (uint32_t)(s * C + c);   // chain id = sample * n_contigs + contig
            check_rc(chain_record_fields(
                         *x.graph, x.plan, recs[chain].data(), ignore_imputed, with_gl, [&](size_t v) { return !any_column[c] || f.kmer_off[v + 1] == f.kmer_off[v]; },
                         [&](std::vector<GenotypingResult>* full) { return fetch_chain_results(job, chain, f, x.goff, cov_rows[s][c], full, err, sizeof(err)); },
                         (*out)[s][x.name]),
                     err);
        }
}

// the column as bytes: one packed copy, then chain by chain; neither calls nor values are fetched.  text[s] = sample s
void cohort_record_text(pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows, bool ignore_imputed,
                        std::vector<std::map<std::string, RecordText>>* text) {
    const size_t C = chroms.size(), S = cov_rows.size();
    char err[512] = {0};
    add_gl_offsets(chroms);
    std::vector<uint64_t> calls_first, off;
    std::string packed;
    check_rc(job_record_text(job, S * C, ignore_imputed, &calls_first, &off, &packed, err, sizeof(err)), err);
    std::vector<char> any_column(C);
    for (size_t c = 0; c < C; ++c) any_column[c] = any_kept_column(chroms[c].flat);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < C; ++c) {
            const Chromosome& x = chroms[c];
            const FlatContig& f = x.flat;
            const size_t chain = s * C + c;
            if (calls_first[chain + 1] - calls_first[chain] != x.plan.nr_of_records())
                fail("genotype_cohort_record_text: chain " + std::to_string(chain) + " holds other records than its plan's");
            RecordText& t = (*text)[s][x.name];
            t.unique_kmers.resize(f.variant_pos.size());
            for (size_t v = 0; v < t.unique_kmers.size(); ++v) t.unique_kmers[v] = any_column[c] ? (unsigned short)(f.kmer_off[v + 1] - f.kmer_off[v]) : 0;
            check_rc(chain_record_text(
                         job, (uint32_t)chain, x, ignore_imputed, off.data() + calls_first[chain], packed,
                         [&](size_t v) { return !any_column[c] || f.kmer_off[v + 1] == f.kmer_off[v]; },
                         [&](size_t v) { return any_column[c] ? cov_rows[s][c][v] : (uint16_t)0; },
                         [&](std::vector<GenotypingResult>* full) { return fetch_chain_results(job, (uint32_t)chain, f, x.goff, cov_rows[s][c], full, err, sizeof(err)); },
                         t, err, sizeof(err)),
                     err);
        }
}

// the record text, then the lines joined on the device: a prefix per chromosome, one launch, one packed copy
void cohort_record_lines(pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows, bool ignore_imputed,
                         std::map<std::string, RecordLines>* lines) {
    const size_t C = chroms.size(), S = cov_rows.size();
    std::vector<std::map<std::string, RecordText>> text(S);
    cohort_record_text(job, chroms, cov_rows, ignore_imputed, &text);
    char err[512] = {0};
    std::vector<std::vector<std::string>> fixed(C);
    for (size_t c = 0; c < C; ++c) {
        const std::string& name = chroms[c].name;
        const std::vector<unsigned short>& uk = text[0][name].unique_kmers;
        for (size_t s = 1; s < S; ++s)
            if (text[s][name].unique_kmers != uk) fail("genotype_cohort_record_lines: the samples' unique k-mer counts differ on " + name);
        fixed[c] = chroms[c].graph->genotypes_fixed_columns(uk);
        std::vector<uint64_t> poff(fixed[c].size() + 1, 0);
        std::string pbytes;
        for (size_t r = 0; r < fixed[c].size(); ++r) { pbytes += fixed[c][r]; poff[r + 1] = pbytes.size(); }
        check_rc(pg_job_line_prefix(job, (uint32_t)c, poff.data(), pbytes.empty() ? nullptr : pbytes.data(), err, sizeof(err)), err);
    }
    check_rc(pg_job_record_lines(job, err, sizeof(err)), err);
    std::vector<uint64_t> line_first(C + 1, 0), byte_first(C + 1, 0);
    uint64_t n_index = 0;
    check_rc(pg_job_record_lines_first(job, &n_index, nullptr, nullptr, err, sizeof(err)), err);
    if (n_index != C) fail("genotype_cohort_record_lines: the job has " + std::to_string(n_index) + " index contigs, not " + std::to_string(C));
    check_rc(pg_job_record_lines_first(job, nullptr, line_first.data(), byte_first.data(), err, sizeof(err)), err);
    std::vector<uint64_t> loff(line_first.back() + 1, 0);
    std::string lbytes(byte_first.back(), '\0');
    check_rc(pg_job_fetch_record_lines_packed(job, loff.data(), lbytes.empty() ? nullptr : &lbytes[0], lbytes.size(), err, sizeof(err)), err);
    for (size_t c = 0; c < C; ++c) {
        const size_t R = fixed[c].size();
        RecordLines dev;
        dev.off.assign(R + 1, 0);
        if (line_first[c + 1] - line_first[c] == R) {   // (a chromosome without records has no lines on the device)
            for (size_t r = 0; r <= R; ++r) dev.off[r] = loff[line_first[c] + r] - byte_first[c];
            dev.bytes.assign(lbytes, byte_first[c], byte_first[c + 1] - byte_first[c]);
        } else if (R != 0 || line_first[c + 1] != line_first[c]) {
            fail("genotype_cohort_record_lines: chromosome " + std::to_string(c) + " holds other lines than its plan's records");
        }
        std::vector<const RecordText*> texts(S);
        for (size_t s = 0; s < S; ++s) texts[s] = &text[s][chroms[c].name];
        (*lines)[chroms[c].name] = compose_record_lines(fixed[c], texts, dev);
    }
}

}  // namespace

std::vector<std::map<std::string, std::vector<GenotypeCall>>> genotype_cohort_record_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, std::vector<GenotypeCall>>> out(samples.size());
    std::vector<std::map<std::string, RecordFields>> fields(samples.size());
    run_record_cohort(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device,
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) {
                          cohort_record_fields(job, chroms, cov_rows, ignore_imputed, false, &fields);
                      });
    for (size_t s = 0; s < fields.size(); ++s)
        for (auto& kv : fields[s]) out[s][kv.first] = std::move(kv.second.calls);
    return out;
}

std::vector<std::map<std::string, RecordFields>> genotype_cohort_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, RecordFields>> out(samples.size());
    run_record_cohort(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device,
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) {
                          cohort_record_fields(job, chroms, cov_rows, ignore_imputed, true, &out);
                      });
    return out;
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, RecordText>> text(samples.size());
    run_record_cohort(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device,
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) {
                          cohort_record_text(job, chroms, cov_rows, ignore_imputed, &text);
                      });
    return text;
}

std::map<std::string, RecordLines> genotype_cohort_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::map<std::string, RecordLines> lines;
    run_record_cohort(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device,
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) {
                          cohort_record_lines(job, chroms, cov_rows, ignore_imputed, &lines);
                      });
    return lines;
}

// ------------------------------------------------------------------ cohort job, the phasing column per VCF record
namespace {

pg_hmm_params phasing_params(double recombrate, bool uniform, long double effective_N) {
    pg_hmm_params prm = genotyping_params(recombrate, uniform, effective_N);
    prm.run_genotyping = 0; prm.run_phasing = 1;
    return prm;
}

// The host route of one chain: pg_job_fetch's haplotypes, kept flags, k-mer counts and coverage as one GenotypingResult per
// bubble — what HMM(..., false, true, ...) hands out —, printed by Graph::phasing_records; the last column of every line.
int chain_phasing_on_host(pg_job* job, uint32_t chain, const Chromosome& x, bool ignore_imputed, RecordText& out, char* err, size_t errlen) {
    const size_t V = x.flat.variant_pos.size();
    std::vector<uint16_t> hap1(V ? V : 1), hap2(V ? V : 1), n_kmers(V ? V : 1), cov(V ? V : 1);
    std::vector<uint8_t> kept(V ? V : 1);
    pg_contig_result r{};
    r.haplotype_1 = hap1.data(); r.haplotype_2 = hap2.data(); r.kept = kept.data(); r.n_kmers = n_kmers.data(); r.coverage = cov.data();
    const int rc = pg_job_fetch(job, chain, &r, err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<GenotypingResult> results(V);
    for (size_t v = 0; v < V; ++v) {
        if (kept[v]) { results[v].add_first_haplotype_allele(hap1[v]); results[v].add_second_haplotype_allele(hap2[v]); }
        results[v].set_unique_kmers(n_kmers[v]);
        results[v].set_coverage(cov[v]);
    }
    out.off.assign(1, 0);
    out.bytes.clear();
    for (const std::string& line : x.graph->phasing_records(results, ignore_imputed)) {
        out.bytes.append(line, line.rfind('\t') + 1, std::string::npos);
        out.off.push_back(out.bytes.size());
    }
    return PG_OK;
}

// the column as bytes: one packed copy, then chain by chain; no haplotype is fetched except on the host route.  text[s] = sample s
void cohort_phased_text(pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows, bool ignore_imputed,
                        std::vector<std::map<std::string, RecordText>>* text) {
    const size_t C = chroms.size(), S = cov_rows.size();
    char err[512] = {0};
    check_rc(pg_job_phased_text(job, ignore_imputed ? 1 : 0, err, sizeof(err)), err);
    std::vector<uint64_t> rec_first(S * C + 1, 0), text_first(S * C + 1, 0);
    check_rc(pg_job_phased_text_first(job, rec_first.data(), text_first.data(), err, sizeof(err)), err);
    std::vector<uint64_t> off(rec_first.back() + 1, 0);
    std::string packed(text_first.back(), '\0');
    check_rc(pg_job_fetch_phased_text_packed(job, off.data(), packed.empty() ? nullptr : &packed[0], packed.size(), err, sizeof(err)), err);
    for (size_t s = 0; s < S; ++s)
        for (size_t c = 0; c < C; ++c) {
            const Chromosome& x = chroms[c];
            const size_t chain = s * C + c, R = x.plan.nr_of_records();
            RecordText& t = (*text)[s][x.name];
            std::vector<uint16_t> n_kmers, coverage;   // (host memory of the job: no device copy)
            check_rc(fetch_chain_meta(job, (uint32_t)chain, x.flat.variant_pos.size(), &n_kmers, &coverage, nullptr, err, sizeof(err)), err);
            t.unique_kmers.assign(n_kmers.begin(), n_kmers.end());
            if (x.host_route) {
                check_rc(chain_phasing_on_host(job, (uint32_t)chain, x, ignore_imputed, t, err, sizeof(err)), err);
                continue;
            }
            if (rec_first[chain + 1] - rec_first[chain] != R) fail("phase_cohort_record_text: chain " + std::to_string(chain) + " holds other records than its plan's");
            const uint64_t* o = off.data() + rec_first[chain];
            t.off.assign(R + 1, 0);
            for (size_t q = 0; q <= R; ++q) t.off[q] = o[q] - o[0];
            t.bytes.assign(packed, o[0], o[R] - o[0]);
        }
}

// The phased text formed and left on the device, then the lines joined there: a prefix per chromosome, one launch, ONE packed
// copy — of the lines.  No text comes to the host: every record has one, so no line is the host's to compose.  UK is what
// pg_job_fetch reports (host memory of the job).  Only the chains of a chromosome on the host route are fetched and printed here.
void cohort_phased_lines(pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows, bool ignore_imputed,
                         std::map<std::string, RecordLines>* lines) {
    const size_t C = chroms.size(), S = cov_rows.size();
    char err[512] = {0};
    check_rc(pg_job_phased_text(job, ignore_imputed ? 1 : 0, err, sizeof(err)), err);
    std::vector<std::vector<std::string>> fixed(C);
    for (size_t c = 0; c < C; ++c) {
        const std::string& name = chroms[c].name;
        const size_t V = chroms[c].flat.variant_pos.size();
        std::vector<uint16_t> first, n_kmers, coverage;
        for (size_t s = 0; s < S; ++s) {
            check_rc(fetch_chain_meta(job, (uint32_t)(s * C + c), V, s ? &n_kmers : &first, &coverage, nullptr, err, sizeof(err)), err);
            if (s && n_kmers != first) fail("phase_cohort_record_lines: the samples' unique k-mer counts differ on " + name);
        }
        fixed[c] = chroms[c].graph->phasing_fixed_columns(std::vector<unsigned short>(first.begin(), first.end()));
        if (chroms[c].host_route) continue;
        std::vector<uint64_t> poff(fixed[c].size() + 1, 0);
        std::string pbytes;
        for (size_t r = 0; r < fixed[c].size(); ++r) { pbytes += fixed[c][r]; poff[r + 1] = pbytes.size(); }
        check_rc(pg_job_phased_line_prefix(job, (uint32_t)c, poff.data(), pbytes.empty() ? nullptr : pbytes.data(), err, sizeof(err)), err);
    }
    check_rc(pg_job_phased_lines(job, err, sizeof(err)), err);
    std::vector<uint64_t> line_first(C + 1, 0), byte_first(C + 1, 0);
    uint64_t n_index = 0;
    check_rc(pg_job_phased_lines_first(job, &n_index, nullptr, nullptr, err, sizeof(err)), err);
    if (n_index != C) fail("phase_cohort_record_lines: the job has " + std::to_string(n_index) + " index contigs, not " + std::to_string(C));
    check_rc(pg_job_phased_lines_first(job, nullptr, line_first.data(), byte_first.data(), err, sizeof(err)), err);
    std::vector<uint64_t> loff(line_first.back() + 1, 0);
    std::string lbytes(byte_first.back(), '\0');
    check_rc(pg_job_fetch_phased_lines_packed(job, loff.data(), lbytes.empty() ? nullptr : &lbytes[0], lbytes.size(), err, sizeof(err)), err);
    for (size_t c = 0; c < C; ++c) {
        const size_t R = fixed[c].size();
        RecordLines& out = (*lines)[chroms[c].name];
        if (chroms[c].host_route) {   // no line on the device: every one is composed from the samples' columns formed here
            std::vector<RecordText> text(S);
            std::vector<const RecordText*> texts(S);
            for (size_t s = 0; s < S; ++s) {
                check_rc(chain_phasing_on_host(job, (uint32_t)(s * C + c), chroms[c], ignore_imputed, text[s], err, sizeof(err)), err);
                texts[s] = &text[s];
            }
            RecordLines none;
            none.off.assign(R + 1, 0);
            out = compose_record_lines(fixed[c], texts, none);
            continue;
        }
        if (line_first[c + 1] - line_first[c] != R) fail("phase_cohort_record_lines: chromosome " + std::to_string(c) + " holds other lines than its plan's records");
        out.off.assign(R + 1, 0);
        for (size_t r = 0; r <= R; ++r) out.off[r] = loff[line_first[c] + r] - byte_first[c];
        out.bytes.assign(lbytes, byte_first[c], byte_first[c + 1] - byte_first[c]);
    }
}

}  // namespace

std::vector<std::map<std::string, RecordText>> phase_cohort_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, std::vector<unsigned short>* only_paths, double recombrate, bool uniform,
    long double effective_N, int device, bool ignore_imputed) {
    std::vector<std::map<std::string, RecordText>> text(samples.size());
    run_record_cohort(chromosomes, graphs, samples, probabilities, only_paths, phasing_params(recombrate, uniform, effective_N), device, "phase_cohort_record_text",
                      [](const Graph& g) { return g.has_undefined_reference_allele(); },
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) { cohort_phased_text(job, chroms, cov_rows, ignore_imputed, &text); });
    return text;
}

std::map<std::string, RecordLines> phase_cohort_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, std::vector<unsigned short>* only_paths, double recombrate, bool uniform,
    long double effective_N, int device, bool ignore_imputed) {
    std::map<std::string, RecordLines> lines;
    run_record_cohort(chromosomes, graphs, samples, probabilities, only_paths, phasing_params(recombrate, uniform, effective_N), device, "phase_cohort_record_lines",
                      [](const Graph& g) { return g.has_undefined_reference_allele(); },
                      [&](pg_job* job, std::vector<Chromosome>& chroms, const CoverageRows& cov_rows) { cohort_phased_lines(job, chroms, cov_rows, ignore_imputed, &lines); });
    return lines;
}

// ------------------------------------------------------------------ path subsets, the sample column per VCF record
std::map<std::string, SampledRecordFields> genotype_subsets_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<std::vector<unsigned short>>& subsets, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N,
    int device, bool ignore_imputed) {
    std::map<std::string, SampledRecordFields> out;
    if (subsets.empty()) fail("genotype_subsets_record_fields: no subsets of paths");
    if (chromosomes.empty()) return out;
    // the graphs first: nothing runs for a chromosome without one
    std::vector<const Graph*> graph;
    std::vector<RecordPlan> plans;
    for (auto& kv : chromosomes) {
        graph.push_back(&graph_of(graphs, kv.first, kv.second.size(), "genotype_subsets_record_fields"));
        plans.push_back(graph.back()->record_plan());
    }
    SubsetsRun R;
    R.run(chromosomes, subsets, probabilities, recombrate, uniform, effective_N, device);
    pg_job* const job = R.job.get();
    const size_t C = R.C, S = R.S;
    int rc = PG_OK;
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {   // the plan of a group is that of its first chain's index contig
        const pg_record_plan view = plans[c].view();
        rc = pg_job_record_plan(job, (uint32_t)(c * S), &view, R.err, sizeof(R.err));
    }
    if (rc == PG_OK) rc = pg_job_combined_record_calls(job, R.err, sizeof(R.err));
    if (rc == PG_OK) rc = pg_job_combined_record_gl(job, R.err, sizeof(R.err));
    check_rc(rc, R.err);
    // all records with one synchronisation, all GL values with another
    std::vector<std::vector<pg_call>> recs(C);
    std::vector<pg_call*> ptrs(C, nullptr);
    std::vector<pg_gl*> gl_ptrs(C, nullptr);
    for (size_t c = 0; c < C; ++c) {
        RecordFields& fields = out[R.names[c]].fields;
        recs[c].resize(plans[c].nr_of_records());
        ptrs[c] = recs[c].empty() ? nullptr : recs[c].data();
        fields.gl_off = record_gl_offsets(plans[c], "pg_record_gl_offsets refused the record plan");
        fields.gl.resize(fields.gl_off.back());
        gl_ptrs[c] = fields.gl.empty() ? nullptr : fields.gl.data();
    }
    check_rc(pg_job_fetch_combined_record_calls_all(job, ptrs.data(), R.err, sizeof(R.err)), R.err);
    check_rc(pg_job_fetch_combined_record_gl_all(job, gl_ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) {
        SampledRecordFields& f = out[R.names[c]];
        std::vector<uint16_t> n_kmers, cov;
        R.first_chain_meta(c, &n_kmers, &cov);
        f.unique_kmers.assign(n_kmers.begin(), n_kmers.end());
        f.coverage.assign(cov.begin(), cov.end());
        rc = chain_record_fields(
            *graph[c], plans[c], recs[c].data(), ignore_imputed, true, [&](size_t v) { return n_kmers[v] == 0; },
            [&](std::vector<GenotypingResult>* full) {   // what the device deferred: from the chains' own bins, added up on the host
                *full = R.combined_on_host(c);
                for (size_t v = 0; v < full->size(); ++v) {
                    (*full)[v].set_unique_kmers(n_kmers[v]);
                    (*full)[v].set_coverage(cov[v]);
                }
                return (int)PG_OK;
            },
            f.fields);
        check_rc(rc, R.err);
    }
    return out;
}

// ------------------------------------------------------------------ cohort job fed by the device counter
std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_reads(
    UniqueKmersMap& index, const std::string& prefix, const std::vector<std::string>& readfiles, const std::vector<size_t>& kmer_coverages,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch) {
    const size_t C = index.unique_kmers.size(), S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_reads: one k-mer coverage per read file");
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (C == 0 || S == 0) return out;
    const size_t B = std::max<size_t>(1, std::min(batch, S));
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    const std::vector<Chromosome> chroms = index_chromosomes(index.unique_kmers);
    // the job is made with the index's own numbers in every sample's place; every sample that is run is filled first
    std::vector<const uint16_t*> count_row(C), cov_row(C);
    for (size_t c = 0; c < C; ++c) { count_row[c] = chroms[c].flat.batch.kmer_count; cov_row[c] = chroms[c].flat.batch.coverage; }
    std::vector<pg_sample_counts> rows(B);
    for (pg_sample_counts& r : rows) { r.kmer_count = count_row.data(); r.coverage = cov_row.data(); }
    const Job job = cohort_job(device, chroms, rows, probabilities, genotyping_params(recombrate, uniform, effective_N));
    char err[512] = {0};
    for (size_t s0 = 0; s0 < S; s0 += B) {
        const size_t n = std::min(B, S - s0);   // (a last, shorter batch: the other samples' chains run on what they hold and are not fetched)
        for (size_t s = 0; s < n; ++s) {
            counter.reset_counts();
            counter.count(readfiles[s0 + s]);
            plan.fill_job(job.get(), (uint32_t)s, kmer_coverages[s0 + s]);
        }
        check_rc(pg_job_run(job.get(), nullptr, err, sizeof(err)), err);
        for (size_t s = 0; s < n; ++s)
            for (size_t c = 0; c < C; ++c)
                check_rc(fetch_chain_results(job.get(), (uint32_t)(s * C + c), chroms[c].flat, chroms[c].goff, nullptr, &out[s0 + s][chroms[c].name], err, sizeof(err)),
                         err);
    }
    return out;
}

// ------------------------------------------------------------------ sampled cohort job
namespace {

using Picks = std::vector<std::vector<uint32_t>>;   // [sample * n_contigs + contig], or empty: the caller wants no sampled paths

// the buffers the sampler writes a job's picks to, and their row pointers as pg_sampler_cohort_new[_device] takes them
std::vector<uint32_t*> pick_rows_of(bool wanted, size_t n, const std::vector<Chromosome>& chroms, uint32_t size, Picks* picks) {
    const size_t C = chroms.size();
    picks->assign(wanted ? n * C : 0, {});
    std::vector<uint32_t*> pick_rows(n * C, nullptr);
    for (size_t g = 0; g < picks->size(); ++g) {
        (*picks)[g].assign((size_t)size * chroms[g % C].flat.variant_pos.size() + 1, 0);
        pick_rows[g] = (*picks)[g].data();
    }
    return pick_rows;
}

// a chain's picks as HaplotypeSampler::get_sampled_paths() has them (src/haplotypesampler.cpp:28-44)
void sampled_paths_of(const uint32_t* picks, uint32_t size, size_t V, bool add_reference, SampledPaths* sampled) {
    for (uint32_t i = 0; i < size; ++i) sampled->sampled_paths.emplace_back(picks + (size_t)i * V, picks + (size_t)(i + 1) * V);
    if (add_reference) sampled->sampled_paths.push_back(std::vector<size_t>(V, 0));
}

// The fetch tail of one chain of a sampled cohort job (chain id = sample * n_contigs + contig): the reduced panel back from the
// device (the allele ids of the results are its own), the results over it, and the picks as
// HaplotypeSampler::get_sampled_paths() has them.  `full` = the contig over ALL paths; `coverage` as fetch_chain_results takes it.
// Returns the C ABI's code, its text in `err`.
int fetch_sampled_chain(pg_job* job, uint32_t chain, const FlatContig& full, const uint16_t* coverage, uint32_t size, bool add_reference,
                        const uint32_t* picks, std::vector<GenotypingResult>* results, SampledPaths* sampled, char* err, size_t errlen) {
    const size_t V = full.variant_pos.size();
    FlatContig r;
    uint32_t nv = 0, np = 0;
    uint64_t sk = 0, sa = 0;
    int rc = pg_job_panel_sizes(job, chain, &nv, &np, &sk, &sa);
    if (rc != PG_OK) { std::snprintf(err, errlen, "genotype_cohort_sampled: pg_job_panel_sizes failed"); return rc; }
    r.variant_pos = full.variant_pos;
    if (coverage) r.coverage.assign(coverage, coverage + V);
    else r.coverage.assign(V, 0);
    r.kmer_off.assign(nv + 1, 0); r.allele_off.assign(nv + 1, 0);
    r.kmer_count.assign(sk, 0); r.allele_id.assign(sa, 0); r.allele_flags.assign(sa, 0); r.allele_kmer_off.assign(sa, 0);
    r.allele_kmer_mask.assign(sa, 0); r.path_allele.assign((size_t)nv * np, 0);
    r.paths.resize(V ? np : 0);
    for (size_t p = 0; p < r.paths.size(); ++p) r.paths[p] = (unsigned short)p;
    if (V) {
        rc = pg_job_fetch_panel(job, chain, r.kmer_off.data(), r.kmer_count.data(), r.allele_off.data(), r.allele_id.data(), r.allele_flags.data(),
                                r.allele_kmer_off.data(), r.allele_kmer_mask.data(), r.path_allele.data(), err, errlen);
        if (rc != PG_OK) return rc;
    }
    r.bind();
    std::vector<uint64_t> goff(V + 1, 0);
    pg_hmm_geno_offsets(&r.batch, goff.data());
    rc = fetch_chain_results(job, chain, r, goff, coverage, results, err, errlen);
    if (rc != PG_OK) return rc;
    if (sampled) sampled_paths_of(picks, size, V, add_reference, sampled);
    return PG_OK;
}

// The three tails of a sampled cohort job (made, not yet run; chains = n samples x C chromosomes, every chain its own index
// contig) behind pg_sampler_cohort_new[_device].  `cov_rows` = the samples' own coverages ([n][C]) or null: then what
// pg_job_fetch hands out.  out[s] / sampled[s] (may be null) = sample s of this job.  Each returns the C ABI's code, its text in `err`.

// the run, then per chain the results over its reduced panel
int sampled_job_results(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows* cov_rows, uint32_t size, bool add_reference,
                        const Picks& picks, std::map<std::string, std::vector<GenotypingResult>>* out, std::map<std::string, SampledPaths>* sampled,
                        char* err, size_t errlen) {
    const size_t C = chroms.size();
    int rc = pg_job_run(job, nullptr, err, errlen);
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c)
            rc = fetch_sampled_chain(job, (uint32_t)(s * C + c), chroms[c].flat, cov_rows ? (*cov_rows)[s][c] : nullptr, size, add_reference,
                                     sampled ? picks[s * C + c].data() : nullptr, &out[s][chroms[c].name], sampled ? &sampled[s][chroms[c].name] : nullptr, err,
                                     errlen);
    return rc;
}

// one strided plan per chromosome, checked and uploaded once for all samples, and the run: the start of both record tails
int sampled_job_run_records(pg_job* job, const std::vector<Chromosome>& chroms, char* err, size_t errlen) {
    const size_t C = chroms.size();
    int rc = PG_OK;
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {
        const pg_record_plan view = chroms[c].plan.view();
        rc = pg_job_record_plan_strided(job, (uint32_t)c, (uint32_t)C, &view, err, errlen);
    }
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, errlen);
    return rc;
}

// KC of bubble v of a sampled chain: the sample's own coverage where the chain has a column, else what pg_job_fetch handed out
uint16_t sampled_coverage(const uint16_t* own, uint32_t n_columns, const std::vector<uint16_t>& fetched, size_t v) {
    return own && n_columns > 0 ? own[v] : own ? (uint16_t)0 : fetched[v];
}

// the record calls and GL values, the two packed fetches, and per chain the fields with what the device deferred finished from
// that chain's own reduced panel and bins (fetch_sampled_chain)
int sampled_job_record_fields(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows* cov_rows, uint32_t size, bool add_reference,
                              bool ignore_imputed, const Picks& picks, std::map<std::string, SampledRecordFields>* out,
                              std::map<std::string, SampledPaths>* sampled, char* err, size_t errlen) {
    const size_t C = chroms.size();
    int rc = sampled_job_run_records(job, chroms, err, errlen);
    if (rc == PG_OK) rc = pg_job_record_calls(job, err, errlen);
    if (rc == PG_OK) rc = pg_job_record_gl(job, err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<uint64_t> calls_first(n * C + 1, 0), gl_first(n * C + 1, 0);
    rc = pg_job_record_first(job, calls_first.data(), gl_first.data(), err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<pg_call> recs(calls_first.back());
    std::vector<pg_gl> gls(gl_first.back());
    rc = pg_job_fetch_record_calls_packed(job, recs.data(), recs.size(), err, errlen);
    if (rc == PG_OK) rc = pg_job_fetch_record_gl_packed(job, gls.data(), gls.size(), err, errlen);
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c) {
            const uint32_t chain = (uint32_t)(s * C + c);   // chain id = sample * n_contigs + contig
            const Chromosome& x = chroms[c];
            const size_t V = x.flat.variant_pos.size();
            if (calls_first[chain + 1] - calls_first[chain] != x.plan.nr_of_records() || gl_first[chain + 1] - gl_first[chain] != x.gl_off.back()) {
                std::snprintf(err, errlen, "genotype_cohort_sampled_record_fields: chain %u holds other records than its plan's", chain);
                return PG_ERR_INVALID;
            }
            SampledRecordFields& f = out[s][x.name];
            std::vector<uint16_t> nk, cov;   // per bubble: the reduced panel's k-mer count and the coverage
            uint32_t n_columns = 0;
            rc = fetch_chain_meta(job, chain, V, &nk, &cov, &n_columns, err, errlen);
            if (rc != PG_OK) break;
            const uint16_t* own = cov_rows ? (*cov_rows)[s][c] : nullptr;
            f.unique_kmers.assign(nk.begin(), nk.end());
            f.coverage.resize(V);
            for (size_t v = 0; v < V; ++v) f.coverage[v] = sampled_coverage(own, n_columns, cov, v);
            f.fields.gl_off = x.gl_off;
            f.fields.gl.assign(gls.begin() + gl_first[chain], gls.begin() + gl_first[chain + 1]);
            if (sampled) sampled_paths_of(picks[chain].data(), size, V, add_reference, &sampled[s][x.name]);
            rc = chain_record_fields(
                *x.graph, x.plan, recs.data() + calls_first[chain], ignore_imputed, true, [&](size_t v) { return f.unique_kmers[v] == 0; },
                [&](std::vector<GenotypingResult>* full) {
                    return fetch_sampled_chain(job, chain, x.flat, own, size, add_reference, nullptr, full, nullptr, err, errlen);
                },
                f.fields);
        }
    return rc;
}

// the column as bytes: one packed copy, then chain by chain
int sampled_job_record_text(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows* cov_rows, uint32_t size, bool add_reference,
                            bool ignore_imputed, const Picks& picks, std::map<std::string, RecordText>* text, std::map<std::string, SampledPaths>* sampled,
                            char* err, size_t errlen) {
    const size_t C = chroms.size();
    int rc = sampled_job_run_records(job, chroms, err, errlen);
    std::vector<uint64_t> first, off;
    std::string packed;
    if (rc == PG_OK) rc = job_record_text(job, n * C, ignore_imputed, &first, &off, &packed, err, errlen);
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c) {
            const uint32_t chain = (uint32_t)(s * C + c);
            const Chromosome& x = chroms[c];
            const size_t V = x.flat.variant_pos.size();
            if (first[chain + 1] - first[chain] != x.plan.nr_of_records()) {
                std::snprintf(err, errlen, "genotype_cohort_sampled_record_text: chain %u holds other records than its plan's", chain);
                return PG_ERR_INVALID;
            }
            std::vector<uint16_t> nk, cov;
            uint32_t n_columns = 0;
            rc = fetch_chain_meta(job, chain, V, &nk, &cov, &n_columns, err, errlen);
            if (rc != PG_OK) break;
            const uint16_t* own = cov_rows ? (*cov_rows)[s][c] : nullptr;
            RecordText& t = text[s][x.name];
            t.unique_kmers.assign(nk.begin(), nk.end());
            if (sampled) sampled_paths_of(picks[chain].data(), size, V, add_reference, &sampled[s][x.name]);
            rc = chain_record_text(
                job, chain, x, ignore_imputed, off.data() + first[chain], packed, [&](size_t v) { return t.unique_kmers[v] == 0; },
                [&](size_t v) { return sampled_coverage(own, n_columns, cov, v); },
                [&](std::vector<GenotypingResult>* full) {
                    return fetch_sampled_chain(job, chain, x.flat, own, size, add_reference, nullptr, full, nullptr, err, errlen);
                },
                t, err, errlen);
        }
    return rc;
}

// whole lines: the text stays on the device, ONE slotted prefix per chromosome is shared by its chains, one
// launch joins every chain's lines with its own UK, one packed copy brings them.  Only a chain with a line the device left to
// the host has its counts and its text fetched: the text is finished as sampled_job_record_text finishes it, the lines are
// composed over a prefix formed with that chain's UK.
int sampled_job_record_lines(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows* cov_rows, uint32_t size, bool add_reference,
                             bool ignore_imputed, const Picks& picks, std::map<std::string, RecordLines>* lines, std::map<std::string, SampledPaths>* sampled,
                             char* err, size_t errlen) {
    const size_t C = chroms.size();
    int rc = sampled_job_run_records(job, chroms, err, errlen);
    if (rc == PG_OK) rc = pg_job_record_text(job, ignore_imputed ? 1 : 0, err, errlen);
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {
        std::vector<uint32_t> slot;
        const std::vector<std::string> fixed = chroms[c].graph->genotypes_fixed_columns_slotted(&slot);
        std::vector<uint64_t> poff(fixed.size() + 1, 0);
        std::string pbytes;
        for (size_t r = 0; r < fixed.size(); ++r) { pbytes += fixed[r]; poff[r + 1] = pbytes.size(); }
        slot.push_back(0);   // (never empty: a null pointer means a plain prefix)
        rc = pg_job_line_prefix_strided(job, (uint32_t)c, (uint32_t)C, poff.data(), pbytes.empty() ? nullptr : pbytes.data(), slot.data(), err, errlen);
    }
    if (rc == PG_OK) rc = pg_job_record_lines(job, err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<uint64_t> line_first(n * C + 1, 0), byte_first(n * C + 1, 0), text_first(n * C + 1, 0);
    uint64_t n_index = 0;
    rc = pg_job_record_lines_first(job, &n_index, nullptr, nullptr, err, errlen);
    if (rc == PG_OK && n_index != n * C) {
        std::snprintf(err, errlen, "genotype_cohort_sampled_record_lines: the job has %llu index contigs, not %zu", (unsigned long long)n_index, n * C);
        return PG_ERR_INVALID;
    }
    if (rc == PG_OK) rc = pg_job_record_lines_first(job, nullptr, line_first.data(), byte_first.data(), err, errlen);
    if (rc == PG_OK) rc = pg_job_record_text_first(job, text_first.data(), err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<uint64_t> loff(line_first.back() + 1, 0);
    std::string lbytes(byte_first.back(), '\0');
    rc = pg_job_fetch_record_lines_packed(job, loff.data(), lbytes.empty() ? nullptr : &lbytes[0], lbytes.size(), err, errlen);
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c) {
            const uint32_t chain = (uint32_t)(s * C + c);   // chain id = sample * n_contigs + contig: an index contig of its own
            const Chromosome& x = chroms[c];
            const size_t V = x.flat.variant_pos.size(), R = x.plan.nr_of_records();
            RecordLines dev;
            dev.off.assign(R + 1, 0);
            if (line_first[chain + 1] - line_first[chain] == R) {   // (a chromosome without records has no lines on the device)
                for (size_t r = 0; r <= R; ++r) dev.off[r] = loff[line_first[chain] + r] - byte_first[chain];
                dev.bytes.assign(lbytes, byte_first[chain], byte_first[chain + 1] - byte_first[chain]);
            } else if (R != 0 || line_first[chain + 1] != line_first[chain]) {
                std::snprintf(err, errlen, "genotype_cohort_sampled_record_lines: chain %u holds other lines than its plan's records", chain);
                return PG_ERR_INVALID;
            }
            if (sampled) sampled_paths_of(picks[chain].data(), size, V, add_reference, &sampled[s][x.name]);
            bool whole = true;
            for (size_t r = 0; r < R; ++r) whole = whole && dev.off[r + 1] != dev.off[r];
            if (whole) { lines[s][x.name] = std::move(dev); continue; }
            // a line is left to the host: this chain's counts and text, finished, and the prefix with its UK
            std::vector<uint16_t> nk, cov;
            uint32_t n_columns = 0;
            rc = fetch_chain_meta(job, chain, V, &nk, &cov, &n_columns, err, errlen);
            if (rc != PG_OK) break;
            std::vector<uint64_t> toff(R + 1, 0);
            std::string tbytes(text_first[chain + 1] - text_first[chain], '\0');
            rc = pg_job_fetch_record_text(job, chain, toff.data(), tbytes.empty() ? nullptr : &tbytes[0], tbytes.size(), err, errlen);
            if (rc != PG_OK) break;
            const uint16_t* own = cov_rows ? (*cov_rows)[s][c] : nullptr;
            RecordText t;
            t.unique_kmers.assign(nk.begin(), nk.end());
            rc = chain_record_text(
                job, chain, x, ignore_imputed, toff.data(), tbytes, [&](size_t v) { return t.unique_kmers[v] == 0; },
                [&](size_t v) { return sampled_coverage(own, n_columns, cov, v); },
                [&](std::vector<GenotypingResult>* full) {
                    return fetch_sampled_chain(job, chain, x.flat, own, size, add_reference, nullptr, full, nullptr, err, errlen);
                },
                t, err, errlen);
            if (rc != PG_OK) break;
            lines[s][x.name] = compose_record_lines(x.graph->genotypes_fixed_columns(t.unique_kmers), {&t}, dev);
        }
    return rc;
}

// ---- the sampled-panel VCF: tails of the same shape; they need no run and no picks

// The host route of one chain: its reduced panel's kmer_off and path_allele back from the device, SampledPanels from them,
// Graph::sampled_panel_records.  Per record the whole line; uk (may be null) = the panel's count per bubble.
int panel_chain_on_host(pg_job* job, uint32_t chain, const Chromosome& x, std::vector<std::string>* lines, std::vector<unsigned short>* uk, char* err,
                        size_t errlen) {
    const size_t V = x.flat.variant_pos.size();
    uint32_t nv = 0, np = 0;
    int rc = pg_job_panel_sizes(job, chain, &nv, &np, nullptr, nullptr);
    if (rc != PG_OK || nv != V) { std::snprintf(err, errlen, "sample_cohort_panel_text: pg_job_panel_sizes failed for chain %u", chain); return rc != PG_OK ? rc : PG_ERR_INVALID; }
    std::vector<uint32_t> koff(V + 1, 0);
    std::vector<uint16_t> pa(V * np, 0);
    if (V) rc = pg_job_fetch_panel(job, chain, koff.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, pa.data(), err, errlen);
    if (rc != PG_OK) return rc;
    std::vector<SampledPanel> panels(V);
    for (size_t v = 0; v < V; ++v) {
        panels[v].path_to_allele.assign(pa.begin() + v * np, pa.begin() + (v + 1) * np);
        panels[v].unique_kmers = (unsigned short)(koff[v + 1] - koff[v]);
    }
    *lines = x.graph->sampled_panel_records(panels);
    if (uk) {
        uk->resize(V);
        for (size_t v = 0; v < V; ++v) (*uk)[v] = (unsigned short)panels[v].unique_kmers;
    }
    return PG_OK;
}

// One strided plan per chromosome that takes the device route, and the text formed.  A chromosome whose graph has a REF of
// undefined sequence gets no plan (the plan calls REF defined, the host prints `.` for a haplotype on it); a panel of more
// paths than the device forms sends every chromosome down the host route.  host[c]: chromosome c is the host's.
int sampled_job_panel_begin(pg_job* job, const std::vector<Chromosome>& chroms, std::vector<char>* host, char* err, size_t errlen) {
    const size_t C = chroms.size();
    host->assign(C, 0);
    int rc = PG_OK;
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {
        if (chroms[c].graph->has_undefined_reference_allele()) { (*host)[c] = 1; continue; }
        const pg_record_plan view = chroms[c].plan.view();
        rc = pg_job_record_plan_strided(job, (uint32_t)c, (uint32_t)C, &view, err, errlen);
    }
    if (rc == PG_OK) rc = pg_job_panel_text(job, err, errlen);
    if (rc == PG_ERR_UNSUPPORTED) {   // (more than 64 paths: nothing was formed)
        host->assign(C, 1);
        rc = PG_OK;
    }
    return rc;
}

// the haplotype columns as bytes: one packed copy of the text, one of the records' UK, then chain by chain
int sampled_job_panel_text(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows*, uint32_t, bool, bool, const Picks&,
                           std::map<std::string, RecordText>* text, std::map<std::string, SampledPaths>*, char* err, size_t errlen) {
    const size_t C = chroms.size();
    std::vector<char> host;
    int rc = sampled_job_panel_begin(job, chroms, &host, err, errlen);
    if (rc != PG_OK) return rc;
    const bool any_device = std::find(host.begin(), host.end(), 0) != host.end();
    std::vector<uint64_t> rfirst(n * C + 1, 0), tfirst(n * C + 1, 0), off(1, 0);
    std::vector<uint16_t> uk;
    std::string packed;
    if (any_device) {
        rc = pg_job_panel_text_first(job, rfirst.data(), tfirst.data(), err, errlen);
        if (rc != PG_OK) return rc;
        off.assign(rfirst.back() + 1, 0);
        packed.assign(tfirst.back(), '\0');
        uk.assign(rfirst.back(), 0);
        rc = pg_job_fetch_panel_text_packed(job, off.data(), packed.empty() ? nullptr : &packed[0], packed.size(), err, errlen);
        if (rc == PG_OK) rc = pg_job_fetch_panel_uk_packed(job, uk.empty() ? nullptr : uk.data(), uk.size(), err, errlen);
    }
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c) {
            const uint32_t chain = (uint32_t)(s * C + c);
            const Chromosome& x = chroms[c];
            const size_t V = x.flat.variant_pos.size(), R = x.plan.nr_of_records();
            RecordText& t = text[s][x.name];
            t.off.assign(R + 1, 0);
            if (host[c]) {   // the lines less their fixed columns and the tab behind them
                std::vector<std::string> lines;
                rc = panel_chain_on_host(job, chain, x, &lines, &t.unique_kmers, err, errlen);
                if (rc != PG_OK) break;
                const std::vector<std::string> fixed = x.graph->sampled_panel_fixed_columns(t.unique_kmers);
                for (size_t r = 0; r < R; ++r) { t.bytes.append(lines[r], fixed[r].size() + 1, std::string::npos); t.off[r + 1] = t.bytes.size(); }
                continue;
            }
            if (rfirst[chain + 1] - rfirst[chain] != R) {
                std::snprintf(err, errlen, "sample_cohort_panel_text: chain %u holds other records than its plan's", chain);
                return PG_ERR_INVALID;
            }
            for (size_t r = 0; r <= R; ++r) t.off[r] = off[rfirst[chain] + r] - tfirst[chain];
            t.bytes.assign(packed, tfirst[chain], tfirst[chain + 1] - tfirst[chain]);
            t.unique_kmers.resize(V);
            for (size_t v = 0; v < V; ++v) t.unique_kmers[v] = uk[rfirst[chain] + x.plan.rec_off[v]];   // (every bubble has a record)
        }
    return rc;
}

// whole lines: the text stays on the device, ONE slotted prefix per chromosome is shared by its chains, one launch joins every
// chain's lines with its panel's own UK, one packed copy brings them
int sampled_job_panel_lines(pg_job* job, size_t n, const std::vector<Chromosome>& chroms, const CoverageRows*, uint32_t, bool, bool, const Picks&,
                            std::map<std::string, RecordLines>* lines, std::map<std::string, SampledPaths>*, char* err, size_t errlen) {
    const size_t C = chroms.size();
    std::vector<char> host;
    int rc = sampled_job_panel_begin(job, chroms, &host, err, errlen);
    if (rc != PG_OK) return rc;
    const bool any_device = std::find(host.begin(), host.end(), 0) != host.end();
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {
        if (host[c]) continue;
        std::vector<uint32_t> slot;
        const std::vector<std::string> fixed = chroms[c].graph->sampled_panel_fixed_columns_slotted(&slot);
        std::vector<uint64_t> poff(fixed.size() + 1, 0);
        std::string pbytes;
        for (size_t r = 0; r < fixed.size(); ++r) { pbytes += fixed[r]; poff[r + 1] = pbytes.size(); }
        slot.push_back(0);   // (never empty: a null pointer means a plain prefix)
        rc = pg_job_panel_line_prefix_strided(job, (uint32_t)c, (uint32_t)C, poff.data(), pbytes.empty() ? nullptr : pbytes.data(), slot.data(), err, errlen);
    }
    std::vector<uint64_t> line_first(n * C + 1, 0), byte_first(n * C + 1, 0), loff(1, 0);
    std::string lbytes;
    if (rc == PG_OK && any_device) {
        rc = pg_job_panel_lines(job, err, errlen);
        uint64_t n_index = 0;
        if (rc == PG_OK) rc = pg_job_panel_lines_first(job, &n_index, nullptr, nullptr, err, errlen);
        if (rc == PG_OK && n_index != n * C) {
            std::snprintf(err, errlen, "sample_cohort_panel_lines: the job has %llu index contigs, not %zu", (unsigned long long)n_index, n * C);
            return PG_ERR_INVALID;
        }
        if (rc == PG_OK) rc = pg_job_panel_lines_first(job, nullptr, line_first.data(), byte_first.data(), err, errlen);
        if (rc != PG_OK) return rc;
        loff.assign(line_first.back() + 1, 0);
        lbytes.assign(byte_first.back(), '\0');
        rc = pg_job_fetch_panel_lines_packed(job, loff.data(), lbytes.empty() ? nullptr : &lbytes[0], lbytes.size(), err, errlen);
    }
    for (size_t s = 0; s < n && rc == PG_OK; ++s)
        for (size_t c = 0; c < C && rc == PG_OK; ++c) {
            const uint32_t chain = (uint32_t)(s * C + c);   // chain id = sample * n_contigs + contig: an index contig of its own
            const Chromosome& x = chroms[c];
            const size_t R = x.plan.nr_of_records();
            RecordLines& out = lines[s][x.name];
            out.off.assign(R + 1, 0);
            if (host[c]) {
                std::vector<std::string> host_lines;
                rc = panel_chain_on_host(job, chain, x, &host_lines, nullptr, err, errlen);
                if (rc != PG_OK) break;
                for (size_t r = 0; r < R; ++r) { out.bytes += host_lines[r]; out.bytes += '\n'; out.off[r + 1] = out.bytes.size(); }
                continue;
            }
            if (line_first[chain + 1] - line_first[chain] == R) {   // (a chromosome without records has no lines on the device)
                for (size_t r = 0; r <= R; ++r) out.off[r] = loff[line_first[chain] + r] - byte_first[chain];
                out.bytes.assign(lbytes, byte_first[chain], byte_first[chain + 1] - byte_first[chain]);
            } else if (R != 0 || line_first[chain + 1] != line_first[chain]) {
                std::snprintf(err, errlen, "sample_cohort_panel_lines: chain %u holds other lines than its plan's records", chain);
                return PG_ERR_INVALID;
            }
        }
    return rc;
}

// One sampled cohort job from the samples' counts on the host (`who`: the caller's name in a refusal), then
// `tail(job, cov_rows, picks, err, errlen)` on the made job: one of the three tails above; it returns the C ABI's code.
template <class Tail>
void sampled_cohort(const std::vector<Chromosome>& chroms, const std::vector<SampleCounts>& samples, const char* who, size_t panel_size,
                    bool add_reference, unsigned short allele_penalty, long double sampling_effective_N, ProbabilityTable* probabilities, double recombrate,
                    bool uniform, long double effective_N, int device, bool want_picks, Tail tail) {
    const SampleRows rows = sample_rows(samples, chroms, who);
    Picks picks;
    const std::vector<uint32_t*> pick_rows = pick_rows_of(want_picks, samples.size(), chroms, (uint32_t)panel_size, &picks);
    const std::vector<pg_contig_batch> index = batches_of(chroms);
    const pg_hmm_params prm = genotyping_params(recombrate, uniform, effective_N);
    char err[1024] = {0};
    pg_job* made = nullptr;
    int rc = pg_sampler_cohort_new(device, (uint32_t)index.size(), index.data(), (uint32_t)samples.size(), rows.rows.data(), (uint32_t)panel_size,
                                   add_reference ? 1 : 0, recombrate, sampling_effective_N, allele_penalty, probabilities->handle(), &prm,
                                   want_picks ? pick_rows.data() : nullptr, nullptr, &made, err, sizeof(err));
    const Job job(made);
    if (rc == PG_OK) rc = tail(made, &rows.cov_rows, picks, err, sizeof(err));
    check_rc(rc, err);
}

// The sampled cohort fed by the device counter: per batch of up to `batch` samples one pg_sampler_counts the count plan fills
// on the device, one job made from it, then `tail(job, s0, n, picks, err, errlen)` for the samples s0 .. s0 + n of this job.
template <class Tail>
void sampled_cohort_batches(DeviceKmerCounter& counter, DeviceCountPlan& plan, const std::vector<Chromosome>& chroms, const std::vector<std::string>& readfiles,
                            const std::vector<size_t>& kmer_coverages, const char* who, size_t panel_size, bool add_reference, unsigned short allele_penalty,
                            long double sampling_effective_N, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N,
                            int device, size_t batch, bool want_picks, Tail tail) {
    const size_t C = chroms.size(), S = readfiles.size();
    const size_t B = std::max<size_t>(1, std::min(batch, S));
    const std::vector<pg_contig_batch> batches = batches_of(chroms);
    std::vector<uint64_t> n_kmers(C);
    std::vector<uint32_t> n_variants(C);
    for (size_t c = 0; c < C; ++c) {
        n_kmers[c] = chroms[c].flat.kmer_count.size();
        n_variants[c] = (uint32_t)chroms[c].flat.variant_pos.size();
    }
    const pg_hmm_params prm = genotyping_params(recombrate, uniform, effective_N);
    char err[1024] = {0};
    auto check_batch = [&](int rc) {   // (a batch that does not fit: the caller's remedy is a smaller one, it is never split here)
        if (rc == PG_ERR_NOMEM) fail(std::string(err) + " (" + who + ": lower `batch`)");
        check_rc(rc, err);
    };
    for (size_t s0 = 0; s0 < S; s0 += B) {
        const size_t n = std::min(B, S - s0);
        pg_sampler_counts* made_counts = nullptr;
        int rc = pg_sampler_counts_new(device, (uint32_t)C, n_kmers.data(), n_variants.data(), (uint32_t)n, &made_counts, err, sizeof(err));
        SamplerCounts counts(made_counts);
        check_batch(rc);
        std::vector<pg_sample_counts> rows(n);
        for (size_t s = 0; s < n; ++s) {
            uint16_t* const* d_k = nullptr;
            uint16_t* const* d_c = nullptr;
            check_rc(pg_sampler_counts_rows(counts.get(), (uint32_t)s, &d_k, &d_c, err, sizeof(err)), err);
            counter.reset_counts();
            counter.count(readfiles[s0 + s]);
            plan.fill_device(kmer_coverages[s0 + s], d_k, d_c);
            rows[s].kmer_count = d_k;
            rows[s].coverage = d_c;
        }
        Picks picks;
        const std::vector<uint32_t*> pick_rows = pick_rows_of(want_picks, n, chroms, (uint32_t)panel_size, &picks);
        pg_job* made = nullptr;
        rc = pg_sampler_cohort_new_device(device, (uint32_t)C, batches.data(), (uint32_t)n, rows.data(), (uint32_t)panel_size, add_reference ? 1 : 0,
                                          recombrate, sampling_effective_N, allele_penalty, probabilities->handle(), &prm,
                                          want_picks ? pick_rows.data() : nullptr, nullptr, &made, err, sizeof(err));
        const Job job(made);
        counts.reset();   // (the job does not reference the arrays)
        if (rc == PG_OK) rc = tail(made, s0, n, picks, err, sizeof(err));
        check_batch(rc);
    }
}

// genotype_cohort_sampled_record_fields and _record_text: one sampled cohort job, then `record_tail`: sampled_job_record_fields
// or sampled_job_record_text, whose `Out` is what comes back per sample and chromosome
template <class Out, class RecordTail>
std::vector<std::map<std::string, Out>> sampled_cohort_records(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled, RecordTail record_tail) {
    const size_t S = samples.size();
    std::vector<std::map<std::string, Out>> out(S);
    if (sampled) sampled->assign(S, {});
    if (chromosomes.empty() || S == 0) return out;
    const std::vector<Chromosome> chroms = record_chromosomes(chromosomes, graphs, "genotype_cohort_sampled_record_fields");
    sampled_cohort(chroms, samples, "genotype_cohort_sampled_record_fields", panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                   recombrate, uniform, effective_N, device, sampled != nullptr,
                   [&](pg_job* job, const CoverageRows* cov_rows, const Picks& picks, char* err, size_t errlen) {
                       return record_tail(job, S, chroms, cov_rows, (uint32_t)panel_size, add_reference, ignore_imputed, picks, out.data(),
                                          sampled ? sampled->data() : nullptr, err, errlen);
                   });
    return out;
}

// genotype_cohort_sampled_reads_record_fields and _record_text: the batches of genotype_cohort_sampled_reads, `record_tail` per job
template <class Out, class RecordTail>
std::vector<std::map<std::string, Out>> sampled_reads_records(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled, RecordTail record_tail) {
    const size_t S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_sampled_reads_record_fields: one k-mer coverage per read file");
    std::vector<std::map<std::string, Out>> out(S);
    if (sampled) sampled->assign(S, {});
    if (index.unique_kmers.empty() || S == 0) return out;
    const std::vector<Chromosome> chroms = record_chromosomes(index.unique_kmers, graphs, "genotype_cohort_sampled_reads_record_fields");
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    sampled_cohort_batches(counter, plan, chroms, readfiles, kmer_coverages, "genotype_cohort_sampled_reads_record_fields", panel_size, add_reference,
                           allele_penalty, sampling_effective_N, probabilities, recombrate, uniform, effective_N, device, batch, sampled != nullptr,
                           [&](pg_job* job, size_t s0, size_t n, const Picks& picks, char* err, size_t errlen) {
                               return record_tail(job, n, chroms, nullptr, (uint32_t)panel_size, add_reference, ignore_imputed, picks, out.data() + s0,
                                                  sampled ? sampled->data() + s0 : nullptr, err, errlen);
                           });
    return out;
}

}  // namespace

std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_sampled(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<SampleCounts>& samples,
    size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(samples.size());
    if (sampled) sampled->assign(samples.size(), {});
    if (chromosomes.empty() || samples.empty()) return out;
    const std::vector<Chromosome> chroms = index_chromosomes(chromosomes);
    sampled_cohort(chroms, samples, "genotype_cohort_sampled", panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities, recombrate, uniform,
                   effective_N, device, sampled != nullptr, [&](pg_job* job, const CoverageRows* cov_rows, const Picks& picks, char* err, size_t errlen) {
                       return sampled_job_results(job, samples.size(), chroms, cov_rows, (uint32_t)panel_size, add_reference, picks, out.data(),
                                                  sampled ? sampled->data() : nullptr, err, errlen);
                   });
    return out;
}

std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_cohort_records<SampledRecordFields>(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                                       recombrate, uniform, effective_N, device, ignore_imputed, sampled, sampled_job_record_fields);
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_cohort_records<RecordText>(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                              recombrate, uniform, effective_N, device, ignore_imputed, sampled, sampled_job_record_text);
}

std::vector<std::map<std::string, RecordLines>> genotype_cohort_sampled_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_cohort_records<RecordLines>(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                               recombrate, uniform, effective_N, device, ignore_imputed, sampled, sampled_job_record_lines);
}

std::vector<std::map<std::string, RecordText>> sample_cohort_panel_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    return sampled_cohort_records<RecordText>(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                              recombrate, uniform, effective_N, device, false, nullptr, sampled_job_panel_text);
}

std::vector<std::map<std::string, RecordLines>> sample_cohort_panel_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    return sampled_cohort_records<RecordLines>(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                               recombrate, uniform, effective_N, device, false, nullptr, sampled_job_panel_lines);
}

std::vector<std::map<std::string, RecordText>> sample_cohort_reads_panel_text(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch) {
    return sampled_reads_records<RecordText>(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N,
                                             probabilities, recombrate, uniform, effective_N, device, batch, false, nullptr, sampled_job_panel_text);
}

std::vector<std::map<std::string, RecordLines>> sample_cohort_reads_panel_lines(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch) {
    return sampled_reads_records<RecordLines>(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N,
                                              probabilities, recombrate, uniform, effective_N, device, batch, false, nullptr, sampled_job_panel_lines);
}

// ------------------------------------------------------------------ sampled cohort job fed by the device counter
std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_sampled_reads(
    UniqueKmersMap& index, const std::string& prefix, const std::vector<std::string>& readfiles, const std::vector<size_t>& kmer_coverages,
    size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    const size_t S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_sampled_reads: one k-mer coverage per read file");
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (sampled) sampled->assign(S, {});
    if (index.unique_kmers.empty() || S == 0) return out;
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    const std::vector<Chromosome> chroms = index_chromosomes(index.unique_kmers);
    sampled_cohort_batches(counter, plan, chroms, readfiles, kmer_coverages, "genotype_cohort_sampled_reads", panel_size, add_reference, allele_penalty,
                           sampling_effective_N, probabilities, recombrate, uniform, effective_N, device, batch, sampled != nullptr,
                           [&](pg_job* job, size_t s0, size_t n, const Picks& picks, char* err, size_t errlen) {
                               return sampled_job_results(job, n, chroms, nullptr, (uint32_t)panel_size, add_reference, picks, out.data() + s0,
                                                          sampled ? sampled->data() + s0 : nullptr, err, errlen);
                           });
    return out;
}

std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_reads_record_fields(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_reads_records<SampledRecordFields>(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty,
                                                      sampling_effective_N, probabilities, recombrate, uniform, effective_N, device, batch, ignore_imputed, sampled,
                                                      sampled_job_record_fields);
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_reads_record_text(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_reads_records<RecordText>(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N,
                                             probabilities, recombrate, uniform, effective_N, device, batch, ignore_imputed, sampled, sampled_job_record_text);
}

std::vector<std::map<std::string, RecordLines>> genotype_cohort_sampled_reads_record_lines(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_reads_records<RecordLines>(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N,
                                              probabilities, recombrate, uniform, effective_N, device, batch, ignore_imputed, sampled, sampled_job_record_lines);
}

}  // namespace pangenie
