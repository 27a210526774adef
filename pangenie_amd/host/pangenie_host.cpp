// pangenie_host.cpp — see pangenie_host.hpp.  Host containers + the HMM adapter over the C ABI.
#include "pangenie_host.hpp"
#include "kmer_counts.hpp"
#include "graph_io.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <fstream>
#include <limits>
#include <iomanip>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_set>

namespace pangenie {

namespace {
thread_local int g_device = 0;
[[noreturn]] void fail(const std::string& msg) { throw std::runtime_error(msg); }
void check_rc(int rc, const char* err) {
    if (rc != PG_OK) fail(err && err[0] ? std::string(err) : ("pangenie_hmm error " + std::to_string(rc)));
}
}  // namespace

// ------------------------------------------------------------------ KmerPath
// behaviour: reference src/kmerpath.cpp:13-48 (window 32), src/kmerpath16.cpp (window 16)
void KmerPath::set_position(unsigned short index) {
    if (kmers_ == 0) offset_ = index;  // first k-mer fixes the window
    const unsigned lo = offset_, hi = offset_ + window_;
    if (index < lo || index >= hi) fail("KmerPath::KmerPath: index is invalid");
    kmers_ |= (uint32_t(1) << (index - offset_));
}
unsigned int KmerPath::get_position(unsigned short index) const {
    const unsigned lo = offset_, hi = offset_ + window_;
    if (index < lo || index >= hi) return 0;
    return (kmers_ >> (index - offset_)) & 1u;
}
size_t KmerPath::nr_kmers() const { return (size_t)__builtin_popcount(kmers_); }
std::string KmerPath::convert_to_string() const {
    std::string s;
    for (unsigned i = 0; i < offset_ + window_; ++i) s += get_position((unsigned short)i) ? '1' : '0';
    return s;
}
std::ostream& operator<<(std::ostream& os, const KmerPath& p) { return os << p.convert_to_string(); }

// ------------------------------------------------------------------ CopyNumber
// behaviour: reference src/copynumber.cpp:10-58
CopyNumber::CopyNumber() : p_{1.0L, 0.0L, 0.0L} {}
CopyNumber::CopyNumber(long double a, long double b, long double c) : p_{a, b, c} {}
CopyNumber::CopyNumber(long double cn_0, long double cn_1, long double cn_2, long double reg) {
    const long double sum = cn_0 + cn_1 + cn_2 + 3.0L * reg;
    p_[0] = (cn_0 + reg) / sum;
    p_[1] = (cn_1 + reg) / sum;
    p_[2] = 1.0L - p_[0] - p_[1];
}
long double CopyNumber::get_probability_of(int cn) const {
    if (cn < 0 || cn > 2) fail("CopyNumber::get_probability_of: Invalid copy number: " + std::to_string(cn));
    return p_[cn];
}
bool CopyNumber::operator==(const CopyNumber& o) const { return p_[0] == o.p_[0] && p_[1] == o.p_[1] && p_[2] == o.p_[2]; }
bool CopyNumber::operator!=(const CopyNumber& o) const { return !(*this == o); }

// ------------------------------------------------------------------ ProbabilityTable
// the long double table lives in the C ABI object so that host and device see the same entries
ProbabilityTable::ProbabilityTable() : t_(pg_table_create_default()) {}
ProbabilityTable::ProbabilityTable(unsigned short cov_min, unsigned short cov_max, unsigned short count_max, long double reg)
    : t_(pg_table_create(cov_min, cov_max, count_max, reg)) {}
ProbabilityTable& ProbabilityTable::operator=(ProbabilityTable&& o) noexcept {
    if (this != &o) { pg_table_destroy(t_); t_ = o.t_; o.t_ = nullptr; }
    return *this;
}
ProbabilityTable::~ProbabilityTable() { pg_table_destroy(t_); }
CopyNumber ProbabilityTable::get_probability(unsigned short cov, unsigned short count) const {
    long double p[3];
    pg_table_get(t_, cov, count, p);
    return CopyNumber(p[0], p[1], p[2]);
}
void ProbabilityTable::modify_probability(unsigned short cov, unsigned short count, CopyNumber prob) {
    if (pg_table_modify(t_, cov, count, prob.get_probability_of(0), prob.get_probability_of(1), prob.get_probability_of(2)) != PG_OK)
        fail("ProbabilityTable::modify_probability: no precomputed values for these parameters.");
}

// ------------------------------------------------------------------ UniqueKmers
template <bool BI>
void UniqueKmersT<BI>::check_allele(unsigned short a, const char* where) const {
    if (BI && a != 0 && a != 1) fail(std::string(where) + ": provided alleles need to be either 0 or 1 (biallelic).");
}
template <bool BI>
UniqueKmersT<BI>::UniqueKmersT(size_t variant_position, std::vector<unsigned short>& alleles)
    : variant_pos_(variant_position), local_coverage_(0), path_to_allele_(alleles.size()) {
    for (size_t i = 0; i < alleles.size(); ++i) {
        check_allele(alleles[i], BI ? "BiallelicUniqueKmers::BiallelicUniqueKmers" : "MultiallelicUniqueKmers");
        path_to_allele_[i] = alleles[i];
        alleles_[alleles[i]];  // every allele carried by a path gets an entry
    }
}
template <bool BI>
void UniqueKmersT<BI>::insert_kmer(unsigned short readcount, std::vector<unsigned short>& allele_ids) {
    const size_t index = counts_.size();
    for (unsigned short a : allele_ids) check_allele(a, "BiallelicUniqueKmers::insert_kmer");
    counts_.push_back(readcount);
    for (unsigned short a : allele_ids) alleles_[a].kmer_path.set_position((unsigned short)index);  // creates the allele if new
}
template <bool BI>
bool UniqueKmersT<BI>::kmer_on_path(size_t kmer_index, size_t path_index) const {
    if (path_index >= path_to_allele_.size()) fail("UniqueKmers::kmer_on_path: path_index " + std::to_string(path_index) + " does not exist.");
    if (kmer_index >= counts_.size()) fail("UniqueKmers::kmer_on_path: requested kmer index: " + std::to_string(kmer_index) + " does not exist.");
    return alleles_.at(path_to_allele_[path_index]).kmer_path.get_position((unsigned short)kmer_index) > 0;
}
template <bool BI>
bool UniqueKmersT<BI>::kmer_on_allele(size_t kmer_index, size_t allele_id) const {
    return alleles_.at((unsigned short)(BI ? (allele_id != 0) : allele_id)).kmer_path.get_position((unsigned short)kmer_index);
}
template <bool BI>
unsigned short UniqueKmersT<BI>::get_readcount_of(size_t kmer_index) {
    if (kmer_index >= counts_.size()) fail("UniqueKmers::get_readcount_of: requested kmer index: " + std::to_string(kmer_index) + " does not exist.");
    return counts_[kmer_index];
}
template <bool BI>
void UniqueKmersT<BI>::update_readcount(size_t kmer_index, unsigned short new_count) {
    if (kmer_index >= counts_.size()) fail("UniqueKmers::update_readcount: requested kmer index: " + std::to_string(kmer_index) + " does not exist.");
    counts_[kmer_index] = new_count;
}
template <bool BI>
void UniqueKmersT<BI>::get_path_ids(std::vector<unsigned short>& p, std::vector<unsigned short>& a, std::vector<unsigned short>* only_include) {
    if (only_include) {
        for (unsigned short id : *only_include)
            if (id < path_to_allele_.size()) { p.push_back(id); a.push_back(path_to_allele_[id]); }
    } else {
        for (size_t i = 0; i < path_to_allele_.size(); ++i) { p.push_back((unsigned short)i); a.push_back(path_to_allele_[i]); }
    }
}
template <bool BI>
void UniqueKmersT<BI>::get_allele_ids(std::vector<unsigned short>& a) {
    for (auto& kv : alleles_) a.push_back(kv.first);
}
template <bool BI>
void UniqueKmersT<BI>::get_defined_allele_ids(std::vector<unsigned short>& a) {
    for (auto& kv : alleles_)
        if (!kv.second.is_undefined) a.push_back(kv.first);
}
template <bool BI>
std::map<unsigned short, int> UniqueKmersT<BI>::kmers_on_alleles() const {
    std::map<unsigned short, int> r;
    for (auto& kv : alleles_) r[kv.first] = (int)kv.second.kmer_path.nr_kmers();
    return r;
}
template <bool BI>
unsigned short UniqueKmersT<BI>::kmers_on_allele(unsigned short allele_id) const {
    check_allele(allele_id, "BiallelicUniqueKmers::kmers_on_allele");
    return (unsigned short)alleles_.at(allele_id).kmer_path.nr_kmers();
}
template <bool BI>
unsigned short UniqueKmersT<BI>::present_kmers_on_allele(unsigned short allele_id) const {
    check_allele(allele_id, "BiallelicUniqueKmers::present_kmers_on_allele");
    const KmerPath& kp = alleles_.at(allele_id).kmer_path;
    unsigned short n = 0;
    for (size_t i = 0; i < counts_.size(); ++i)
        if (counts_[i] >= 3 && kp.get_position((unsigned short)i)) ++n;  // read-supported = count >= 3
    return n;
}
template <bool BI>
float UniqueKmersT<BI>::fraction_present_kmers_on_allele(unsigned short allele_id) const {
    const unsigned short total = kmers_on_allele(allele_id);
    return total > 0 ? present_kmers_on_allele(allele_id) / (float)total : 1.0f;
}
template <bool BI>
bool UniqueKmersT<BI>::is_undefined_allele(unsigned short allele_id) const {
    check_allele(allele_id, "BiallelicUniqueKmers::is_undefined_allele");
    auto it = alleles_.find(allele_id);
    return it != alleles_.end() && it->second.is_undefined;
}
template <bool BI>
void UniqueKmersT<BI>::set_undefined_allele(unsigned short allele_id) {
    auto it = alleles_.find(allele_id);
    if ((BI && allele_id > 1) || it == alleles_.end())
        fail("UniqueKmers::set_undefined_allele: allele_id " + std::to_string(allele_id) + " does not exist.");
    it->second.is_undefined = true;
}
template <bool BI>
unsigned short UniqueKmersT<BI>::get_allele(unsigned short path_id) const {
    if (path_id >= path_to_allele_.size()) fail("UniqueKmers:get_allele: index out of bounds.");
    return path_to_allele_[path_id];
}
template <bool BI>
std::pair<unsigned short, uint32_t> UniqueKmersT<BI>::kmer_bits(unsigned short allele_id) const {
    const KmerPath& kp = alleles_.at(allele_id).kmer_path;
    return {kp.offset(), kp.mask()};
}
// keep only the given paths; k-mers that sit on none of the surviving alleles are dropped
// (behaviour: reference src/biallelicuniquekmers.cpp:223-260, src/multiallelicuniquekmers.cpp:196-232)
template <bool BI>
void UniqueKmersT<BI>::update_paths(std::vector<unsigned short>& path_ids) {
    std::vector<unsigned short> new_p2a(path_ids.size());
    std::map<unsigned short, AlleleInfo> kept;
    for (size_t i = 0; i < path_ids.size(); ++i) {
        const unsigned short a = get_allele(path_ids[i]);
        new_p2a[i] = a;
        kept[a] = alleles_[a];
    }
    std::map<size_t, std::vector<unsigned short>> kmer_to_alleles;
    std::vector<unsigned short> undefined;
    for (auto& kv : kept) {
        for (size_t k = 0; k < counts_.size(); ++k)
            if (kv.second.kmer_path.get_position((unsigned short)k)) kmer_to_alleles[k].push_back(kv.first);
        if (kv.second.is_undefined) undefined.push_back(kv.first);
    }
    const std::vector<unsigned short> old_counts = counts_;
    path_to_allele_ = new_p2a;
    alleles_.clear();
    for (unsigned short a : new_p2a) alleles_[a];
    counts_.clear();
    for (unsigned short a : undefined) set_undefined_allele(a);
    for (auto& kv : kmer_to_alleles) insert_kmer(old_counts[kv.first], kv.second);
}
template class UniqueKmersT<true>;
template class UniqueKmersT<false>;

// ------------------------------------------------------------------ ColumnIndexer
// behaviour: reference src/columnindexer.cpp:8-78
ColumnIndexer::ColumnIndexer(std::vector<std::shared_ptr<UniqueKmers>>* unique_kmers, std::vector<unsigned short>* only_paths)
    : unique_kmers_(unique_kmers) {
    for (size_t v = 0; v < unique_kmers->size(); ++v) {
        std::vector<unsigned short> p, a;
        UniqueKmers& uk = *unique_kmers->at(v);
        uk.get_path_ids(p, a, only_paths);
        if (p.empty()) fail("HMM::index_columns: column " + std::to_string(v) + " is not covered by any paths.");
        if (v == 0) paths_ = p;
        bool any_alt = false;
        for (unsigned short al : a)
            if (al != 0 && !uk.is_undefined_allele(al)) any_alt = true;
        if (any_alt) columns_.push_back(v);
    }
}
size_t ColumnIndexer::get_variant_id(size_t c) const {
    if (c >= columns_.size()) fail("ColumnIndexer::get_variant_id: column index does not exist.");
    return columns_[c];
}
unsigned short ColumnIndexer::get_path(unsigned short i) const {
    if (i >= paths_.size()) fail("ColumnIndexer::get_path: path_index does not exist.");
    return paths_[i];
}
unsigned short ColumnIndexer::get_allele(unsigned short path_index, size_t column_index) const {
    const unsigned short path = get_path(path_index);
    if (column_index >= columns_.size()) fail("ColumnIndex::get_allele: column_index does not exist.");
    return unique_kmers_->at(columns_[column_index])->get_allele(path);
}
std::pair<unsigned short, unsigned short> ColumnIndexer::get_path_ids_at(size_t position) const {
    const size_t n = paths_.size();
    if (position >= n * n) fail("ColumnIndexer::get_path_ids_at: index out of bounds.");
    return {(unsigned short)(position / n), (unsigned short)(position % n)};
}

// ------------------------------------------------------------------ GenotypingResult
// behaviour: reference src/genotypingresult.cpp
GenotypingResult::GenotypingResult() : haplotype_1_(0), haplotype_2_(0), local_coverage_(0), unique_kmers_(0) {}
static std::pair<unsigned short, unsigned short> ordered(unsigned short a, unsigned short b) {
    return a < b ? std::make_pair(a, b) : std::make_pair(b, a);
}
void GenotypingResult::add_to_likelihood(unsigned short a1, unsigned short a2, long double value) {
    genotype_to_likelihood_[ordered(a1, a2)] += value;
}
long double GenotypingResult::get_genotype_likelihood(unsigned short a1, unsigned short a2) const {
    auto it = genotype_to_likelihood_.find(ordered(a1, a2));
    return it == genotype_to_likelihood_.end() ? 0.0L : it->second;
}
std::vector<long double> GenotypingResult::get_all_likelihoods(size_t nr_alleles) const {
    std::vector<long double> out(nr_alleles * (nr_alleles + 1) / 2, 0.0L);
    for (auto& kv : genotype_to_likelihood_) {
        const size_t a1 = kv.first.first, a2 = kv.first.second;
        const size_t idx = a2 * (a2 + 1) / 2 + a1;  // VCF genotype ordering
        if (idx >= out.size()) fail("GenotypeResult::get_all_likelihoods: genotype does not match number of alleles.");
        out[idx] = kv.second;
    }
    return out;
}
GenotypingResult GenotypingResult::get_specific_likelihoods(std::vector<unsigned short>& alleles) const {
    GenotypingResult res;
    std::map<unsigned short, unsigned short> index;
    for (unsigned short i = 0; i < alleles.size(); ++i) index[alleles[i]] = i;
    long double sum = 0.0L;
    for (auto& kv : genotype_to_likelihood_) {
        auto i1 = index.find(kv.first.first), i2 = index.find(kv.first.second);
        if (i1 == index.end() || i2 == index.end()) continue;
        if (haplotype_1_ == kv.first.first) res.haplotype_1_ = i1->second;
        if (haplotype_2_ == kv.first.second) res.haplotype_2_ = i2->second;
        res.add_to_likelihood(i1->second, i2->second, kv.second);
        sum += kv.second;
    }
    if (sum > 0) res.divide_likelihoods_by(sum);
    return res;
}
size_t GenotypingResult::get_genotype_quality(unsigned short a1, unsigned short a2) const {
    long double sum = 0.0L;
    for (auto& kv : genotype_to_likelihood_) sum += kv.second;
    if (fabsl(sum - 1) > 0.0000000001L)
        fail("GenotypingResult::get_genotype_quality: genotype quality can only be computed from normalized likelihoods.");
    const long double prob_wrong = 1.0L - get_genotype_likelihood(a1, a2);
    if (prob_wrong > 0.0L) return (size_t)(-10 * log10l(prob_wrong));
    return 10000;
}
void GenotypingResult::divide_likelihoods_by(long double value) {
    for (auto& kv : genotype_to_likelihood_) kv.second = kv.second / value;
}
std::pair<int, int> GenotypingResult::get_likeliest_genotype() const {
    if (genotype_to_likelihood_.empty()) return {-1, -1};
    long double best_value = 0.0L;
    std::pair<unsigned short, unsigned short> best(0, 0);
    for (auto& kv : genotype_to_likelihood_)
        if (kv.second >= best_value) { best_value = kv.second; best = kv.first; }
    for (auto& kv : genotype_to_likelihood_)
        if (kv.first != best && fabsl(kv.second - best_value) < 0.0000000001L) return {-1, -1};  // no unique maximum
    if (best_value > 0.0L) return {best.first, best.second};
    return {-1, -1};
}
void GenotypingResult::combine(GenotypingResult& other) {
    for (auto& kv : other.genotype_to_likelihood_) genotype_to_likelihood_[kv.first] += kv.second;
}
void GenotypingResult::normalize() {
    long double sum = 0.0L;
    for (auto& kv : genotype_to_likelihood_) sum += kv.second;
    if (sum > 0) divide_likelihoods_by(sum);
}
std::ostream& operator<<(std::ostream& os, const GenotypingResult& r) {
    os << "haplotype allele 1: " << r.haplotype_1_ << "\nhaplotype allele 2: " << r.haplotype_2_
       << "\nlocal coverage: " << r.local_coverage_ << "\nnr of unique kmers: " << r.unique_kmers_ << "\n";
    for (auto& kv : r.genotype_to_likelihood_) os << kv.first.first << "/" << kv.first.second << ": " << (double)kv.second << "\n";
    return os;
}

template <bool B>
UniqueKmersT<B>::UniqueKmersT(const Raw& raw)
    : variant_pos_(raw.variant_pos), local_coverage_(raw.local_coverage), counts_(raw.counts), path_to_allele_(raw.path_to_allele) {
    for (auto& kv : raw.alleles) {
        AlleleInfo info;
        info.kmer_path = KmerPath(B ? 16u : 32u, kv.second.offset, kv.second.mask);
        info.is_undefined = kv.second.is_undefined;
        alleles_[kv.first] = info;
    }
}
template <bool B>
typename UniqueKmersT<B>::Raw UniqueKmersT<B>::raw() const {
    Raw r;
    r.variant_pos = variant_pos_; r.local_coverage = local_coverage_; r.counts = counts_; r.path_to_allele = path_to_allele_;
    for (auto& kv : alleles_) {
        RawAllele a;
        a.offset = kv.second.kmer_path.offset(); a.mask = kv.second.kmer_path.mask(); a.is_undefined = kv.second.is_undefined;
        r.alleles[kv.first] = a;
    }
    return r;
}
template UniqueKmersT<true>::UniqueKmersT(const Raw&);
template UniqueKmersT<false>::UniqueKmersT(const Raw&);
template UniqueKmersT<true>::Raw UniqueKmersT<true>::raw() const;
template UniqueKmersT<false>::Raw UniqueKmersT<false>::raw() const;

// ------------------------------------------------------------------ VCF sample column
std::string genotype_field(const GenotypingResult& result, std::vector<unsigned short>& defined_alleles, size_t nr_alleles, bool ignore_imputed) {
    GenotypingResult tmp = result;
    if (tmp.contains_no_likelihoods()) tmp.add_to_likelihood(0, 0, 1.0);   // reference src/graph.cpp:225-227
    const size_t nr_missing = nr_alleles - defined_alleles.size();
    GenotypingResult gl = nr_missing > 0 ? tmp.get_specific_likelihoods(defined_alleles) : tmp;   // :229-233
    nr_alleles = defined_alleles.size();
    std::ostringstream out;
    std::pair<int, int> genotype = gl.get_likeliest_genotype();
    if (ignore_imputed && result.nr_unique_kmers() == 0) genotype = {-1, -1};
    if (genotype.first != -1 && genotype.second != -1)
        out << genotype.first << "/" << genotype.second << ":" << gl.get_genotype_quality((unsigned short)genotype.first, (unsigned short)genotype.second) << ":";
    else
        out << ".:.:";
    std::vector<long double> likelihoods = gl.get_all_likelihoods(nr_alleles);
    if (likelihoods.size() < 3) fail("Graph::write_genotypes_of: too few likelihoods (" + std::to_string(likelihoods.size()) + ") computed");
    out << std::setprecision(4) << std::log10(likelihoods[0]);
    for (size_t j = 1; j < likelihoods.size(); ++j) out << "," << std::setprecision(4) << std::log10(likelihoods[j]);
    out << ":" << result.coverage();
    return out.str();
}

// ------------------------------------------------------------------ flatten
void FlatContig::bind() {
    static const uint16_t z16 = 0; static const uint32_t z32 = 0; static const uint8_t z8 = 0; static const uint64_t z64 = 0;
    batch.n_variants = (uint32_t)variant_pos.size();
    batch.n_paths = (uint32_t)paths.size();
    batch.variant_pos = variant_pos.empty() ? &z64 : variant_pos.data();
    batch.coverage = coverage.empty() ? &z16 : coverage.data();
    batch.kmer_off = kmer_off.data();
    batch.kmer_count = kmer_count.empty() ? &z16 : kmer_count.data();
    batch.allele_off = allele_off.data();
    batch.allele_id = allele_id.empty() ? &z16 : allele_id.data();
    batch.allele_flags = allele_flags.empty() ? &z8 : allele_flags.data();
    batch.allele_kmer_off = allele_kmer_off.empty() ? &z16 : allele_kmer_off.data();
    batch.allele_kmer_mask = allele_kmer_mask.empty() ? &z32 : allele_kmer_mask.data();
    batch.path_allele = path_allele.empty() ? &z16 : path_allele.data();
}

void flatten(std::vector<std::shared_ptr<UniqueKmers>>* unique_kmers, std::vector<unsigned short>* only_paths, FlatContig& f) {
    const size_t V = unique_kmers->size();
    f = FlatContig();
    f.kmer_off.assign(1, 0);
    f.allele_off.assign(1, 0);
    f.variant_pos.reserve(V); f.coverage.reserve(V); f.kmer_off.reserve(V + 1); f.allele_off.reserve(V + 1);
    std::vector<unsigned short> p, a, ids;
    for (size_t v = 0; v < V; ++v) {
        UniqueKmers& uk = *unique_kmers->at(v);
        p.clear(); a.clear(); ids.clear();
        uk.get_path_ids(p, a, only_paths);
        if (p.empty()) fail("HMM::index_columns: column " + std::to_string(v) + " is not covered by any paths.");
        if (v == 0) {  // the selected paths are those of the first variant (ColumnIndexer)
            f.paths = p;
            f.path_allele.reserve(V * p.size()); f.kmer_count.reserve(V * (uk.size() + 4)); f.allele_id.reserve(V * 2);
        }
        f.variant_pos.push_back(uk.get_variant_position());
        f.coverage.push_back(uk.get_coverage());
        for (size_t k = 0; k < uk.size(); ++k) f.kmer_count.push_back(uk.get_readcount_of(k));
        f.kmer_off.push_back((uint32_t)f.kmer_count.size());
        uk.get_allele_ids(ids);
        for (unsigned short id : ids) {
            f.allele_id.push_back(id);
            f.allele_flags.push_back(uk.is_undefined_allele(id) ? 1 : 0);
            auto bits = uk.kmer_bits(id);
            f.allele_kmer_off.push_back(bits.first);
            f.allele_kmer_mask.push_back(bits.second);
        }
        f.allele_off.push_back((uint32_t)f.allele_id.size());
        if (p == f.paths) f.path_allele.insert(f.path_allele.end(), a.begin(), a.end());  // (get_path_ids already gave the alleles)
        else for (unsigned short path : f.paths) f.path_allele.push_back(uk.get_allele(path));
    }
    f.bind();
}

// ------------------------------------------------------------------ device-backed computers
TransitionProbabilityComputer::TransitionProbabilityComputer(size_t from_variant, size_t to_variant, double recomb_rate,
                                                             unsigned short nr_paths, bool uniform, long double effective_N)
    : uniform_(uniform) {
    double out[3];
    char err[256] = {0};
    check_rc(pg_transition_probs(from_variant, to_variant, recomb_rate, nr_paths, uniform ? 1 : 0, effective_N, g_device, out, err, sizeof(err)), err);
    for (int i = 0; i < 3; ++i) probabilities_[i] = out[i];
}
long double TransitionProbabilityComputer::compute_transition_prob(unsigned short p1, unsigned short p2, unsigned short p3, unsigned short p4) {
    if (uniform_) return 1.0L;
    return probabilities_[(p1 != p3) + (p2 != p4)];
}
long double TransitionProbabilityComputer::compute_transition_prob(unsigned short nr_switches) {
    if (uniform_) return 1.0L;
    return probabilities_[nr_switches];
}

EmissionProbabilityComputer::EmissionProbabilityComputer(std::shared_ptr<UniqueKmers> uniquekmers, ProbabilityTable* probabilities) {
    std::vector<std::shared_ptr<UniqueKmers>> one{uniquekmers};
    FlatContig f;
    flatten(&one, nullptr, f);
    allele_ids_.assign(f.allele_id.begin(), f.allele_id.end());
    const size_t A = allele_ids_.size();
    table_.assign(A * A, 0.0L);
    char err[256] = {0};
    int32_t all_zeros = 0;
    check_rc(pg_emission_table(&f.batch, probabilities->handle(), 0, g_device, table_.data(), &all_zeros, err, sizeof(err)), err);
}
long double EmissionProbabilityComputer::get_emission_probability(unsigned short a1, unsigned short a2) const {
    const size_t A = allele_ids_.size();
    size_t s1 = A, s2 = A;
    for (size_t i = 0; i < A; ++i) { if (allele_ids_[i] == a1) s1 = i; if (allele_ids_[i] == a2) s2 = i; }
    if (s1 == A || s2 == A) fail("EmissionProbabilityComputer: unknown allele");
    return table_[s1 * A + s2];
}

// ------------------------------------------------------------------ HMM
void HMM::set_device(int device) { g_device = device; }
int HMM::device_count() { return pg_hmm_device_count(); }

// behaviour of the constructor: reference src/hmm.cpp:25-63 — everything between ColumnIndexer
// and the optional normalisation runs on the GPU behind pg_hmm_genotype_contig().
HMM::HMM(std::vector<std::shared_ptr<UniqueKmers>>* unique_kmers, ProbabilityTable* probabilities, bool run_genotyping,
         bool run_phasing, double recombrate, bool uniform, long double effective_N, std::vector<unsigned short>* only_paths,
         bool normalize_results)
    : genotyping_result_(unique_kmers->size()) {
    // N of these constructors run at a time on the reference's thread-pool workers (src/commands.cpp:949-978): tell the
    // library a call is coming BEFORE the (host-side, size-dependent) flattening, so that whichever worker reaches the
    // device first knows whom to wait for and all of them end up as chains of ONE device job (pg_hmm_announce).
    struct Announcement {
        int device; bool open;
        explicit Announcement(int d) : device(d), open(true) { pg_hmm_announce(d); }
        ~Announcement() { if (open) pg_hmm_retract(device); }
    } announcement(g_device);
    FlatContig f;
    flatten(unique_kmers, only_paths, f);
    const size_t V = f.variant_pos.size();
    std::vector<uint64_t> geno_off(V + 1, 0);
    pg_hmm_geno_offsets(&f.batch, geno_off.data());
    std::vector<double> lik(geno_off[V] ? geno_off[V] : 1);
    std::vector<int32_t> lik_exp(geno_off[V] ? geno_off[V] : 1);  // one exponent per genotype bin
    std::vector<uint8_t> kept(V ? V : 1), present(f.allele_id.size() ? f.allele_id.size() : 1);
    std::vector<uint16_t> n_kmers(V ? V : 1), cov(V ? V : 1), hap1(V ? V : 1), hap2(V ? V : 1);
    // Viterbi on the device (pg_viterbi.hip): at most 64 selected paths (the reference's callers pass at most 30,
    // src/commands.cpp:939); above that the C ABI refuses (PG_ERR_UNSUPPORTED -> std::runtime_error).  There is no host
    // compute path behind this constructor.
    const bool phase_on_device = run_phasing;
    pg_contig_result r{};
    r.lik = lik.data(); r.lik_exp = lik_exp.data(); r.kept = kept.data(); r.allele_present = present.data();
    r.n_kmers = n_kmers.data(); r.coverage = cov.data();
    r.haplotype_1 = hap1.data(); r.haplotype_2 = hap2.data();
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0;
    prm.run_genotyping = run_genotyping ? 1 : 0; prm.run_phasing = phase_on_device ? 1 : 0;
    char err[512] = {0};
    if (run_genotyping || phase_on_device) {
        prm.reserved = PG_CALL_ANNOUNCED;
        announcement.open = false;  // (the call retires the announcement itself)
        check_rc(pg_hmm_genotype_contig(&f.batch, probabilities->handle(), &prm, announcement.device, &r, err, sizeof(err)), err);
    }
    if (run_genotyping) {
        for (size_t v = 0; v < V; ++v) {
            GenotypingResult& g = genotyping_result_[v];
            if (kept[v]) {
                const uint32_t a0 = f.allele_off[v], A = f.allele_off[v + 1] - a0;
                for (uint32_t a = 0; a < A; ++a) {
                    if (!present[a0 + a]) continue;
                    for (uint32_t b = a; b < A; ++b) {
                        if (!present[a0 + b]) continue;
                        const uint64_t idx = geno_off[v] + (uint64_t)a * A - (uint64_t)a * (a - 1) / 2 + (b - a);
                        // the device returns lik[g] * 2^lik_exp[g]; rebuild the reference's long double
                        g.add_to_likelihood(f.allele_id[a0 + a], f.allele_id[a0 + b], ldexpl((long double)lik[idx], lik_exp[idx]));
                    }
                }
            }
            g.set_unique_kmers(n_kmers[v]);
            g.set_coverage(cov[v]);
        }
        if (normalize_results) normalize();  // reference src/hmm.cpp:36-45
    }
    if (phase_on_device) {  // reference src/hmm.cpp:47-49, :144-172
        for (size_t v = 0; v < V; ++v)
            if (kept[v]) {
                genotyping_result_[v].add_first_haplotype_allele(hap1[v]);
                genotyping_result_[v].add_second_haplotype_allele(hap2[v]);
            }
        // (sic: the reference sets these two by COLUMN index, not by variant — src/hmm.cpp:164-165)
        for (size_t c = 0; c < r.n_columns; ++c) {
            genotyping_result_[c].set_unique_kmers((unsigned short)(f.kmer_off[c + 1] - f.kmer_off[c]));
            genotyping_result_[c].set_coverage(f.coverage[c]);
        }
    }
}
// ------------------------------------------------------------------ results of one chain of a job
// vector<GenotypingResult> of one chain from its packed posteriors (reference src/hmm.cpp:364-368, 106-109); kept columns
// and allele presence by the ColumnIndexer rule on the host (src/columnindexer.cpp:24-31).  `coverage` = the chain's own
// local coverages (a cohort's chains share the index, not these).
static std::vector<GenotypingResult> results_of_chain(const FlatContig& f, const uint16_t* coverage, const std::vector<uint64_t>& goff,
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

    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    std::vector<pg_job*> jobs(D, nullptr);
    std::vector<std::string> errors(D);
    std::vector<std::thread> threads;
    for (size_t d = 0; d < D; ++d)
        threads.emplace_back([&, d] {
            if (plan[d].empty()) return;
            std::vector<pg_contig_batch> b;
            for (size_t t : plan[d]) b.push_back(flat[t].batch);
            char err[512] = {0};
            int rc = pg_job_new(devices[d], (uint32_t)b.size(), b.data(), probabilities->handle(), &prm, &jobs[d], err, sizeof(err));
            if (rc == PG_OK) rc = pg_job_run(jobs[d], nullptr, err, sizeof(err));
            if (rc != PG_OK) errors[d] = err[0] ? err : "pangenie_hmm error";
        });
    for (auto& th : threads) th.join();
    auto cleanup = [&] { for (pg_job* j : jobs) if (j) pg_job_destroy(j); };
    for (size_t d = 0; d < D; ++d)
        if (!errors[d].empty()) { cleanup(); fail(errors[d]); }

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
            const int rc = pg_job_fetch(jobs[0], (uint32_t)k, &r, err, sizeof(err));
            if (rc != PG_OK) { cleanup(); check_rc(rc, err); }
            off += goff[plan[0][k]].back();
        }
    } else {
        std::vector<pg_comm*> comms(D, nullptr);
        int rc = pg_comm_init_all((int)D, devices.data(), comms.data(), err, sizeof(err));
        if (rc == PG_OK) rc = pg_hmm_gather_to_host((int)D, comms.data(), jobs.data(), 0, n_lik.data(), lik.data(), lexp.data(), err, sizeof(err));
        for (pg_comm* c : comms) if (c) pg_comm_destroy(c);
        if (rc != PG_OK) { cleanup(); check_rc(rc, err); }
    }
    cleanup();

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
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);
    std::vector<std::vector<uint64_t>> goff(C);
    std::vector<pg_contig_batch> index(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        goff[c].assign(flat[c].variant_pos.size() + 1, 0);
        pg_hmm_geno_offsets(&flat[c].batch, goff[c].data());
        index[c] = flat[c].batch;
        c += 1;
    }
    // per sample the two pointer rows of pg_sample_counts; sizes checked against the index
    static const uint16_t none = 0;
    std::vector<std::vector<const uint16_t*>> count_rows(S, std::vector<const uint16_t*>(C)), cov_rows(S, std::vector<const uint16_t*>(C));
    std::vector<pg_sample_counts> rows(S);
    for (size_t s = 0; s < S; ++s) {
        for (c = 0; c < C; ++c) {
            const auto k = samples[s].kmer_count.find(names[c]), v = samples[s].coverage.find(names[c]);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != flat[c].kmer_count.size() ||
                v->second.size() != flat[c].variant_pos.size())
                fail("genotype_cohort: sample " + std::to_string(s) + " does not fit the index on " + names[c]);
            count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        rows[s].kmer_count = count_rows[s].data();
        rows[s].coverage = cov_rows[s].data();
    }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[512] = {0};
    pg_job* job = nullptr;
    int rc = pg_cohort_new(device, (uint32_t)C, index.data(), (uint32_t)S, rows.data(), probabilities->handle(), &prm, &job, err, sizeof(err));
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
    if (rc != PG_OK) { if (job) pg_job_destroy(job); check_rc(rc, err); }
    for (size_t s = 0; s < S && rc == PG_OK; ++s)
        for (c = 0; c < C && rc == PG_OK; ++c) {
            const uint64_t n = goff[c].back();
            std::vector<double> lik(n ? n : 1);
            std::vector<int32_t> lexp(n ? n : 1);
            pg_contig_result r{};
            r.lik = lik.data(); r.lik_exp = lexp.data();
            rc = pg_job_fetch(job, (uint32_t)(s * C + c), &r, err, sizeof(err));   // chain id = sample * n_contigs + contig
            if (rc == PG_OK) out[s][names[c]] = results_of_chain(flat[c], cov_rows[s][c], goff[c], lik.data(), lexp.data());
        }
    pg_job_destroy(job);
    check_rc(rc, err);
    return out;
}

// ------------------------------------------------------------------ cohort job, calls instead of likelihoods
std::vector<std::map<std::string, std::vector<GenotypeCall>>> genotype_cohort_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<SampleCounts>& samples,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, std::vector<GenotypeCall>>> out(S);
    if (C == 0 || S == 0) return out;
    // (the job is made exactly as genotype_cohort makes it)
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);
    std::vector<std::vector<uint64_t>> goff(C);
    std::vector<pg_contig_batch> index(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        goff[c].assign(flat[c].variant_pos.size() + 1, 0);
        pg_hmm_geno_offsets(&flat[c].batch, goff[c].data());
        index[c] = flat[c].batch;
        c += 1;
    }
    static const uint16_t none = 0;
    std::vector<std::vector<const uint16_t*>> count_rows(S, std::vector<const uint16_t*>(C)), cov_rows(S, std::vector<const uint16_t*>(C));
    std::vector<pg_sample_counts> rows(S);
    for (size_t s = 0; s < S; ++s) {
        for (c = 0; c < C; ++c) {
            const auto k = samples[s].kmer_count.find(names[c]), v = samples[s].coverage.find(names[c]);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != flat[c].kmer_count.size() ||
                v->second.size() != flat[c].variant_pos.size())
                fail("genotype_cohort_calls: sample " + std::to_string(s) + " does not fit the index on " + names[c]);
            count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        rows[s].kmer_count = count_rows[s].data();
        rows[s].coverage = cov_rows[s].data();
    }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[512] = {0};
    pg_job* job = nullptr;
    int rc = pg_cohort_new(device, (uint32_t)C, index.data(), (uint32_t)S, rows.data(), probabilities->handle(), &prm, &job, err, sizeof(err));
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
    if (rc == PG_OK) rc = pg_job_calls(job, err, sizeof(err));
    if (rc != PG_OK) { if (job) pg_job_destroy(job); check_rc(rc, err); }
    // all records with one synchronisation
    std::vector<std::vector<pg_call>> recs(S * C);
    std::vector<pg_call*> ptrs(S * C, nullptr);
    for (size_t i = 0; i < S * C; ++i) {
        recs[i].resize(flat[i % C].variant_pos.size());
        ptrs[i] = recs[i].empty() ? nullptr : recs[i].data();
    }
    rc = pg_job_fetch_calls_all(job, ptrs.data(), err, sizeof(err));
    for (size_t s = 0; s < S && rc == PG_OK; ++s)
        for (c = 0; c < C && rc == PG_OK; ++c) {
            const std::vector<pg_call>& r = recs[s * C + c];   // chain id = sample * n_contigs + contig
            std::vector<GenotypeCall>& calls = out[s][names[c]];
            calls.resize(r.size());
            bool any_deferred = false;
            for (size_t v = 0; v < r.size(); ++v) {
                if (r[v].flags == PG_CALL_OK) { calls[v].allele_1 = r[v].allele_1; calls[v].allele_2 = r[v].allele_2; calls[v].quality = r[v].gq; }
                else if (r[v].flags == PG_CALL_DEFERRED) any_deferred = true;
            }
            if (!any_deferred) continue;
            // the deferred variants of this chain on the host, each from its own bins, through GenotypingResult
            const uint64_t n = goff[c].back();
            std::vector<double> lik(n ? n : 1);
            std::vector<int32_t> lexp(n ? n : 1);
            pg_contig_result res{};
            res.lik = lik.data(); res.lik_exp = lexp.data();
            rc = pg_job_fetch(job, (uint32_t)(s * C + c), &res, err, sizeof(err));
            if (rc != PG_OK) break;
            std::vector<GenotypingResult> full = results_of_chain(flat[c], cov_rows[s][c], goff[c], lik.data(), lexp.data());
            for (size_t v = 0; v < r.size(); ++v) {
                if (r[v].flags != PG_CALL_DEFERRED) continue;
                full[v].normalize();
                const std::pair<int, int> g = full[v].get_likeliest_genotype();
                calls[v].deferred = true;
                if (g.first >= 0 && g.second >= 0) {
                    calls[v].allele_1 = g.first; calls[v].allele_2 = g.second;
                    calls[v].quality = full[v].get_genotype_quality((unsigned short)g.first, (unsigned short)g.second);
                }
            }
        }
    pg_job_destroy(job);
    check_rc(rc, err);
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
    pg_job* job = nullptr;
    char err[512] = {0};
    ~SubsetsRun() { if (job) pg_job_destroy(job); }

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
        pg_hmm_params prm{};
        prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
        int rc = pg_job_new(device, (uint32_t)(C * S), batches.data(), probabilities->handle(), &prm, &job, err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_combine_plan(job, (uint32_t)C, group_off.data(), chains.data(), err, sizeof(err));
        if (rc == PG_OK) rc = pg_job_combine(job, err, sizeof(err));
        check_rc(rc, err);
    }

    // chromosome c on the host route: every subset's chain from its fetched bins, combine_likelihoods in the order of the subsets
    std::vector<GenotypingResult> combined_on_host(size_t c) {
        std::vector<GenotypingResult> total;
        const uint64_t n = goff[c].back();
        std::vector<double> lik(n ? n : 1);
        std::vector<int32_t> lexp(n ? n : 1);
        for (size_t s = 0; s < S; ++s) {
            pg_contig_result res{};
            res.lik = lik.data(); res.lik_exp = lexp.data();
            check_rc(pg_job_fetch(job, (uint32_t)(c * S + s), &res, err, sizeof(err)), err);
            const FlatContig& f = flat[c * S + s];
            static const uint16_t none = 0;
            std::vector<GenotypingResult> one = results_of_chain(f, f.coverage.empty() ? &none : f.coverage.data(), goff[c], lik.data(), lexp.data());
            if (s == 0) total = std::move(one);
            else for (size_t v = 0; v < total.size(); ++v) total[v].combine(one[v]);
        }
        return total;
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
    check_rc(pg_job_fetch_combined_all(R.job, ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) {
        const FlatContig& f = R.flat[c * S];
        const size_t V = f.variant_pos.size();
        std::vector<GenotypingResult>& res = out[R.names[c]];
        res.resize(V);
        // unique_kmers and coverage are those of the first chain (GenotypingResult::combine leaves them alone)
        std::vector<uint16_t> n_kmers(V ? V : 1), cov(V ? V : 1);
        pg_contig_result first{};
        first.n_kmers = n_kmers.data(); first.coverage = cov.data();
        check_rc(pg_job_fetch(R.job, (uint32_t)(c * S), &first, R.err, sizeof(R.err)), R.err);
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
    check_rc(pg_job_combined_calls(R.job, R.err, sizeof(R.err)), R.err);
    const size_t C = R.C, S = R.S;
    std::vector<std::vector<pg_call>> recs(C);
    std::vector<pg_call*> ptrs(C, nullptr);
    for (size_t c = 0; c < C; ++c) {
        recs[c].resize(R.flat[c * S].variant_pos.size());
        ptrs[c] = recs[c].empty() ? nullptr : recs[c].data();
    }
    check_rc(pg_job_fetch_combined_calls_all(R.job, ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) {
        const std::vector<pg_call>& r = recs[c];
        std::vector<GenotypeCall>& calls = out[R.names[c]];
        calls.resize(r.size());
        bool any_deferred = false;
        for (size_t v = 0; v < r.size(); ++v) {
            if (r[v].flags == PG_CALL_OK) { calls[v].allele_1 = r[v].allele_1; calls[v].allele_2 = r[v].allele_2; calls[v].quality = r[v].gq; }
            else if (r[v].flags == PG_CALL_DEFERRED) any_deferred = true;
        }
        if (!any_deferred) continue;
        std::vector<GenotypingResult> full = R.combined_on_host(c);
        for (size_t v = 0; v < r.size(); ++v) {
            if (r[v].flags != PG_CALL_DEFERRED) continue;
            full[v].normalize();
            const std::pair<int, int> g = full[v].get_likeliest_genotype();
            calls[v].deferred = true;
            if (g.first >= 0 && g.second >= 0) {
                calls[v].allele_1 = g.first; calls[v].allele_2 = g.second;
                calls[v].quality = full[v].get_genotype_quality((unsigned short)g.first, (unsigned short)g.second);
            }
        }
    }
    return out;
}

// ------------------------------------------------------------------ cohort job, calls per VCF record
// GT and GQ of one record as genotype_field prints them (graph.cpp:217-273), without the text
static GenotypeCall record_call_on_host(const VcfSite& site) {
    GenotypingResult tmp = site.likelihoods;
    if (tmp.contains_no_likelihoods()) tmp.add_to_likelihood(0, 0, 1.0);
    std::vector<unsigned short> defined = {0};
    for (size_t a = 1; a < site.alleles.size(); ++a)
        if (!site.undefined[a]) defined.push_back((unsigned short)a);
    const GenotypingResult gl = defined.size() < site.alleles.size() ? tmp.get_specific_likelihoods(defined) : tmp;
    GenotypeCall call;
    call.deferred = true;
    const std::pair<int, int> g = gl.get_likeliest_genotype();
    if (g.first >= 0 && g.second >= 0) {
        call.allele_1 = g.first; call.allele_2 = g.second;
        call.quality = gl.get_genotype_quality((unsigned short)g.first, (unsigned short)g.second);
    }
    return call;
}

// the four digits of a long double logarithm as the device stores them: glibc prints the exact decimal expansion
static pg_gl gl_of_log10(long double v) {
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
static void record_gl_on_host(const VcfSite& site, pg_gl* out, size_t n) {
    GenotypingResult tmp = site.likelihoods;
    if (tmp.contains_no_likelihoods()) tmp.add_to_likelihood(0, 0, 1.0);
    std::vector<unsigned short> defined = {0};
    for (size_t a = 1; a < site.alleles.size(); ++a)
        if (!site.undefined[a]) defined.push_back((unsigned short)a);
    const GenotypingResult gl = defined.size() < site.alleles.size() ? tmp.get_specific_likelihoods(defined) : tmp;
    const std::vector<long double> all = gl.get_all_likelihoods(defined.size());
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
static int chain_record_fields(const Graph& graph, const RecordPlan& plan, const pg_call* r, bool ignore_imputed, bool with_gl, NoKmers no_kmers,
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
            if ((r[q].flags & 0xFF) == PG_CALL_OK) { calls[q].allele_1 = r[q].allele_1; calls[q].allele_2 = r[q].allele_2; calls[q].quality = r[q].gq; }
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
static int job_record_text(pg_job* job, size_t n_chains, bool ignore_imputed, std::vector<uint64_t>* calls_first, std::vector<uint64_t>* off,
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
static int chain_record_text(pg_job* job, uint32_t chain, const Graph& graph, const RecordPlan& plan, const std::vector<uint64_t>& gl_off, bool ignore_imputed,
                             const uint64_t* off, const std::string& packed, NoKmers no_kmers, Coverage coverage, Results results, RecordText& out, char* err,
                             size_t errlen) {
    const size_t R = plan.nr_of_records();
    out.off.assign(R + 1, 0);
    for (size_t q = 0; q <= R; ++q) out.off[q] = off[q] - off[0];
    out.bytes.assign(packed, off[0], off[R] - off[0]);
    std::vector<size_t> pending;
    for (size_t q = 0; q < R; ++q)
        if (out.off[q + 1] == out.off[q] && gl_off[q + 1] - gl_off[q] >= 3) pending.push_back(q);
    if (pending.empty()) return PG_OK;
    RecordFields fields;
    fields.gl_off = gl_off;
    fields.gl.resize(gl_off.back());
    std::vector<pg_call> r(R);
    int rc = pg_job_fetch_record_calls(job, chain, r.data(), err, errlen);
    if (rc == PG_OK) rc = pg_job_fetch_record_gl(job, chain, fields.gl.data(), err, errlen);
    if (rc == PG_OK) rc = chain_record_fields(graph, plan, r.data(), ignore_imputed, true, no_kmers, results, fields);
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

// genotype_cohort_record_calls and, `with_gl`, genotype_cohort_record_fields: one job, the calls and the GL values per record;
// with `text` (genotype_cohort_record_text) the column's bytes instead: neither calls nor values are fetched then
static std::vector<std::map<std::string, RecordFields>> cohort_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed, bool with_gl, std::vector<std::map<std::string, RecordText>>* text = nullptr, std::map<std::string, RecordLines>* lines = nullptr) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, RecordFields>> out(S);
    if (text) text->assign(S, {});
    if (C == 0 || S == 0) return out;
    // (the job is made exactly as genotype_cohort makes it)
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);
    std::vector<std::vector<uint64_t>> goff(C);
    std::vector<pg_contig_batch> index(C);
    std::vector<RecordPlan> plans(C);
    std::vector<const Graph*> graph_of(C, nullptr);
    std::vector<char> any_column(C, 0);   // (results_of_chain: a chain without a kept column reports no unique k-mers)
    size_t c = 0;
    for (auto& kv : chromosomes) {
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        goff[c].assign(flat[c].variant_pos.size() + 1, 0);
        pg_hmm_geno_offsets(&flat[c].batch, goff[c].data());
        index[c] = flat[c].batch;
        const auto g = graphs.find(kv.first);
        if (g == graphs.end() || g->second.size() != kv.second.size()) fail("genotype_cohort_record_calls: no graph of " + kv.first + " with the index's bubbles");
        graph_of[c] = &g->second;
        plans[c] = g->second.record_plan();
        const FlatContig& f = flat[c];
        const size_t H = f.paths.size();
        for (size_t v = 0; v < f.variant_pos.size() && !any_column[c]; ++v)
            for (size_t p = 0; p < H && !any_column[c]; ++p) {
                const uint16_t a = f.path_allele[v * H + p];
                for (uint32_t q = f.allele_off[v]; q < f.allele_off[v + 1]; ++q)
                    if (f.allele_id[q] == a && a != 0 && !(f.allele_flags[q] & 1)) any_column[c] = 1;
            }
        c += 1;
    }
    static const uint16_t none = 0;
    std::vector<std::vector<const uint16_t*>> count_rows(S, std::vector<const uint16_t*>(C)), cov_rows(S, std::vector<const uint16_t*>(C));
    std::vector<pg_sample_counts> rows(S);
    for (size_t s = 0; s < S; ++s) {
        for (c = 0; c < C; ++c) {
            const auto k = samples[s].kmer_count.find(names[c]), v = samples[s].coverage.find(names[c]);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != flat[c].kmer_count.size() ||
                v->second.size() != flat[c].variant_pos.size())
                fail("genotype_cohort_record_calls: sample " + std::to_string(s) + " does not fit the index on " + names[c]);
            count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        rows[s].kmer_count = count_rows[s].data();
        rows[s].coverage = cov_rows[s].data();
    }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[512] = {0};
    pg_job* job = nullptr;
    int rc = pg_cohort_new(device, (uint32_t)C, index.data(), (uint32_t)S, rows.data(), probabilities->handle(), &prm, &job, err, sizeof(err));
    for (c = 0; c < C && rc == PG_OK; ++c) {   // one plan per chromosome, whatever the number of samples
        const pg_record_plan view = plans[c].view();
        rc = pg_job_record_plan(job, (uint32_t)c, &view, err, sizeof(err));
    }
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
    if (rc == PG_OK && !text) rc = pg_job_record_calls(job, err, sizeof(err));
    if (rc == PG_OK && with_gl && !text) rc = pg_job_record_gl(job, err, sizeof(err));
    if (rc != PG_OK) { if (job) pg_job_destroy(job); check_rc(rc, err); }
    // the offsets of the GL values hang on the plan alone
    std::vector<std::vector<uint64_t>> gl_off(C);
    for (c = 0; c < C && (with_gl || text); ++c) {
        gl_off[c].assign(plans[c].nr_of_records() + 1, 0);
        const pg_record_plan view = plans[c].view();
        rc = pg_record_gl_offsets(&view, gl_off[c].data());
        if (rc != PG_OK) { pg_job_destroy(job); check_rc(rc, "pg_record_gl_offsets refused the record plan"); }
    }
    // the fetch of a chain's bins, for what the device deferred
    const auto results_of = [&](size_t s, size_t cc, std::vector<GenotypingResult>* full) {
        const uint64_t n = goff[cc].back();
        std::vector<double> lik(n ? n : 1);
        std::vector<int32_t> lexp(n ? n : 1);
        pg_contig_result res{};
        res.lik = lik.data(); res.lik_exp = lexp.data();
        const int code = pg_job_fetch(job, (uint32_t)(s * C + cc), &res, err, sizeof(err));
        if (code == PG_OK) *full = results_of_chain(flat[cc], cov_rows[s][cc], goff[cc], lik.data(), lexp.data());
        return code;
    };
    if (text) {   // the column as bytes: one packed copy, then chain by chain
        std::vector<uint64_t> calls_first, off;
        std::string packed;
        try {
            rc = job_record_text(job, S * C, ignore_imputed, &calls_first, &off, &packed, err, sizeof(err));
            for (size_t s = 0; s < S && rc == PG_OK; ++s)
                for (c = 0; c < C && rc == PG_OK; ++c) {
                    const FlatContig& f = flat[c];
                    const size_t chain = s * C + c;
                    if (calls_first[chain + 1] - calls_first[chain] != plans[c].nr_of_records()) {
                        std::snprintf(err, sizeof(err), "genotype_cohort_record_text: chain %zu holds other records than its plan's", chain);
                        rc = PG_ERR_INVALID;
                        break;
                    }
                    RecordText& t = (*text)[s][names[c]];
                    t.unique_kmers.resize(f.variant_pos.size());
                    for (size_t v = 0; v < t.unique_kmers.size(); ++v) t.unique_kmers[v] = any_column[c] ? (unsigned short)(f.kmer_off[v + 1] - f.kmer_off[v]) : 0;
                    rc = chain_record_text(
                        job, (uint32_t)chain, *graph_of[c], plans[c], gl_off[c], ignore_imputed, off.data() + calls_first[chain], packed,
                        [&](size_t v) { return !any_column[c] || f.kmer_off[v + 1] == f.kmer_off[v]; },
                        [&](size_t v) { return any_column[c] ? cov_rows[s][c][v] : (uint16_t)0; },
                        [&](std::vector<GenotypingResult>* full) { return results_of(s, c, full); }, t, err, sizeof(err));
                }
            if (lines && rc == PG_OK) {   // the lines joined on the device: a prefix per chromosome, one launch, one packed copy
                std::vector<std::vector<std::string>> fixed(C);
                for (c = 0; c < C && rc == PG_OK; ++c) {
                    const std::vector<unsigned short>& uk = (*text)[0][names[c]].unique_kmers;
                    for (size_t s = 1; s < S; ++s)
                        if ((*text)[s][names[c]].unique_kmers != uk) fail("genotype_cohort_record_lines: the samples' unique k-mer counts differ on " + names[c]);
                    fixed[c] = graph_of[c]->genotypes_fixed_columns(uk);
                    std::vector<uint64_t> poff(fixed[c].size() + 1, 0);
                    std::string pbytes;
                    for (size_t r = 0; r < fixed[c].size(); ++r) { pbytes += fixed[c][r]; poff[r + 1] = pbytes.size(); }
                    rc = pg_job_line_prefix(job, (uint32_t)c, poff.data(), pbytes.empty() ? nullptr : pbytes.data(), err, sizeof(err));
                }
                if (rc == PG_OK) rc = pg_job_record_lines(job, err, sizeof(err));
                std::vector<uint64_t> line_first(C + 1, 0), byte_first(C + 1, 0), loff;
                std::string lbytes;
                uint64_t n_index = 0;
                if (rc == PG_OK) rc = pg_job_record_lines_first(job, &n_index, nullptr, nullptr, err, sizeof(err));
                if (rc == PG_OK && n_index != C) { std::snprintf(err, sizeof(err), "genotype_cohort_record_lines: the job has %llu index contigs, not %zu", (unsigned long long)n_index, C); rc = PG_ERR_INVALID; }
                if (rc == PG_OK) rc = pg_job_record_lines_first(job, nullptr, line_first.data(), byte_first.data(), err, sizeof(err));
                if (rc == PG_OK) {
                    loff.assign(line_first.back() + 1, 0);
                    lbytes.assign(byte_first.back(), '\0');
                    rc = pg_job_fetch_record_lines_packed(job, loff.data(), lbytes.empty() ? nullptr : &lbytes[0], lbytes.size(), err, sizeof(err));
                }
                for (c = 0; c < C && rc == PG_OK; ++c) {
                    const size_t R = fixed[c].size();
                    RecordLines dev;
                    dev.off.assign(R + 1, 0);
                    if (line_first[c + 1] - line_first[c] == R) {   // (a chromosome without records has no lines on the device)
                        for (size_t r = 0; r <= R; ++r) dev.off[r] = loff[line_first[c] + r] - byte_first[c];
                        dev.bytes.assign(lbytes, byte_first[c], byte_first[c + 1] - byte_first[c]);
                    } else if (R != 0 || line_first[c + 1] != line_first[c]) {
                        std::snprintf(err, sizeof(err), "genotype_cohort_record_lines: chromosome %zu holds other lines than its plan's records", c);
                        rc = PG_ERR_INVALID;
                        break;
                    }
                    std::vector<const RecordText*> texts(S);
                    for (size_t s = 0; s < S; ++s) texts[s] = &(*text)[s][names[c]];
                    (*lines)[names[c]] = compose_record_lines(fixed[c], texts, dev);
                }
            }
        } catch (...) {
            pg_job_destroy(job);
            throw;
        }
        pg_job_destroy(job);
        check_rc(rc, err);
        return out;
    }
    // all records with one synchronisation
    std::vector<std::vector<pg_call>> recs(S * C);
    std::vector<pg_call*> ptrs(S * C, nullptr);
    for (size_t i = 0; i < S * C; ++i) {
        recs[i].resize(plans[i % C].nr_of_records());
        ptrs[i] = recs[i].empty() ? nullptr : recs[i].data();
    }
    rc = pg_job_fetch_record_calls_all(job, ptrs.data(), err, sizeof(err));
    if (with_gl && rc == PG_OK) {   // ... and all GL values with another
        std::vector<pg_gl*> gl_ptrs(S * C, nullptr);
        for (size_t i = 0; i < S * C; ++i) {
            RecordFields& fields = out[i / C][names[i % C]];
            fields.gl_off = gl_off[i % C];
            fields.gl.resize(fields.gl_off.back());
            gl_ptrs[i] = fields.gl.empty() ? nullptr : fields.gl.data();
        }
        rc = pg_job_fetch_record_gl_all(job, gl_ptrs.data(), err, sizeof(err));
    }
    for (size_t s = 0; s < S && rc == PG_OK; ++s)
        for (c = 0; c < C && rc == PG_OK; ++c) {
            const std::vector<pg_call>& r = recs[s * C + c];   // chain id = sample * n_contigs + contig
            const RecordPlan& plan = plans[c];
            const FlatContig& f = flat[c];
            RecordFields& fields = out[s][names[c]];
            rc = chain_record_fields(
                *graph_of[c], plan, r.data(), ignore_imputed, with_gl,
                [&](size_t v) { return !any_column[c] || f.kmer_off[v + 1] == f.kmer_off[v]; },
                [&](std::vector<GenotypingResult>* full) { return results_of(s, c, full); }, fields);
        }
    pg_job_destroy(job);
    check_rc(rc, err);
    return out;
}

std::vector<std::map<std::string, std::vector<GenotypeCall>>> genotype_cohort_record_calls(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, std::vector<GenotypeCall>>> out(samples.size());
    if (chromosomes.empty()) return out;
    std::vector<std::map<std::string, RecordFields>> fields =
        cohort_record_fields(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device, ignore_imputed, false);
    for (size_t s = 0; s < fields.size(); ++s)
        for (auto& kv : fields[s]) out[s][kv.first] = std::move(kv.second.calls);
    return out;
}

std::vector<std::map<std::string, RecordFields>> genotype_cohort_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    return cohort_record_fields(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device, ignore_imputed, true);
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, RecordText>> text;
    cohort_record_fields(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device, ignore_imputed, true, &text);
    return text;
}

std::map<std::string, RecordLines> genotype_cohort_record_lines(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    bool ignore_imputed) {
    std::vector<std::map<std::string, RecordText>> text;
    std::map<std::string, RecordLines> lines;
    cohort_record_fields(chromosomes, graphs, samples, probabilities, recombrate, uniform, effective_N, device, ignore_imputed, true, &text, &lines);
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
    std::vector<const Graph*> graph_of;
    std::vector<RecordPlan> plans;
    for (auto& kv : chromosomes) {
        const auto g = graphs.find(kv.first);
        if (g == graphs.end() || g->second.size() != kv.second.size()) fail("genotype_subsets_record_fields: no graph of " + kv.first + " with the index's bubbles");
        graph_of.push_back(&g->second);
        plans.push_back(g->second.record_plan());
    }
    SubsetsRun R;
    R.run(chromosomes, subsets, probabilities, recombrate, uniform, effective_N, device);
    const size_t C = R.C, S = R.S;
    int rc = PG_OK;
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {   // the plan of a group is that of its first chain's index contig
        const pg_record_plan view = plans[c].view();
        rc = pg_job_record_plan(R.job, (uint32_t)(c * S), &view, R.err, sizeof(R.err));
    }
    if (rc == PG_OK) rc = pg_job_combined_record_calls(R.job, R.err, sizeof(R.err));
    if (rc == PG_OK) rc = pg_job_combined_record_gl(R.job, R.err, sizeof(R.err));
    check_rc(rc, R.err);
    // all records with one synchronisation, all GL values with another
    std::vector<std::vector<pg_call>> recs(C);
    std::vector<pg_call*> ptrs(C, nullptr);
    std::vector<pg_gl*> gl_ptrs(C, nullptr);
    for (size_t c = 0; c < C; ++c) {
        RecordFields& fields = out[R.names[c]].fields;
        recs[c].resize(plans[c].nr_of_records());
        ptrs[c] = recs[c].empty() ? nullptr : recs[c].data();
        fields.gl_off.assign(plans[c].nr_of_records() + 1, 0);
        const pg_record_plan view = plans[c].view();
        check_rc(pg_record_gl_offsets(&view, fields.gl_off.data()), "pg_record_gl_offsets refused the record plan");
        fields.gl.resize(fields.gl_off.back());
        gl_ptrs[c] = fields.gl.empty() ? nullptr : fields.gl.data();
    }
    check_rc(pg_job_fetch_combined_record_calls_all(R.job, ptrs.data(), R.err, sizeof(R.err)), R.err);
    check_rc(pg_job_fetch_combined_record_gl_all(R.job, gl_ptrs.data(), R.err, sizeof(R.err)), R.err);
    for (size_t c = 0; c < C; ++c) {
        SampledRecordFields& f = out[R.names[c]];
        const size_t V = R.flat[c * S].variant_pos.size();
        // unique_kmers and coverage are those of the first chain (GenotypingResult::combine leaves them alone)
        std::vector<uint16_t> n_kmers(V ? V : 1), cov(V ? V : 1);
        pg_contig_result first{};
        first.n_kmers = n_kmers.data(); first.coverage = cov.data();
        check_rc(pg_job_fetch(R.job, (uint32_t)(c * S), &first, R.err, sizeof(R.err)), R.err);
        f.unique_kmers.assign(n_kmers.begin(), n_kmers.begin() + V);
        f.coverage.assign(cov.begin(), cov.begin() + V);
        rc = chain_record_fields(
            *graph_of[c], plans[c], recs[c].data(), ignore_imputed, true, [&](size_t v) { return n_kmers[v] == 0; },
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
    auto& chromosomes = index.unique_kmers;
    const size_t C = chromosomes.size(), S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_reads: one k-mer coverage per read file");
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (C == 0 || S == 0) return out;
    const size_t B = std::max<size_t>(1, std::min(batch, S));
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);
    std::vector<std::vector<uint64_t>> goff(C);
    std::vector<pg_contig_batch> batches(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {   // (map order: the plan's)
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        goff[c].assign(flat[c].variant_pos.size() + 1, 0);
        pg_hmm_geno_offsets(&flat[c].batch, goff[c].data());
        batches[c] = flat[c].batch;
        c += 1;
    }
    // the job is made with the index's own numbers in every sample's place; every sample that is run is filled first
    std::vector<const uint16_t*> count_row(C), cov_row(C);
    for (c = 0; c < C; ++c) { count_row[c] = flat[c].batch.kmer_count; cov_row[c] = flat[c].batch.coverage; }
    std::vector<pg_sample_counts> rows(B);
    for (pg_sample_counts& r : rows) { r.kmer_count = count_row.data(); r.coverage = cov_row.data(); }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[512] = {0};
    pg_job* job = nullptr;
    int rc = pg_cohort_new(device, (uint32_t)C, batches.data(), (uint32_t)B, rows.data(), probabilities->handle(), &prm, &job, err, sizeof(err));
    if (rc != PG_OK) { if (job) pg_job_destroy(job); check_rc(rc, err); }
    try {
        for (size_t s0 = 0; s0 < S; s0 += B) {
            const size_t n = std::min(B, S - s0);   // (a last, shorter batch: the other samples' chains run on what they hold and are not fetched)
            for (size_t s = 0; s < n; ++s) {
                counter.reset_counts();
                counter.count(readfiles[s0 + s]);
                plan.fill_job(job, (uint32_t)s, kmer_coverages[s0 + s]);
            }
            rc = pg_job_run(job, nullptr, err, sizeof(err));
            for (size_t s = 0; s < n && rc == PG_OK; ++s)
                for (c = 0; c < C && rc == PG_OK; ++c) {
                    const uint64_t nl = goff[c].back();
                    const size_t V = flat[c].variant_pos.size();
                    std::vector<double> lik(nl ? nl : 1);
                    std::vector<int32_t> lexp(nl ? nl : 1);
                    std::vector<uint16_t> cov(V ? V : 1);
                    pg_contig_result r{};
                    r.lik = lik.data(); r.lik_exp = lexp.data(); r.coverage = cov.data();
                    rc = pg_job_fetch(job, (uint32_t)(s * C + c), &r, err, sizeof(err));
                    // (pg_job_fetch hands the coverage out only when the chain has columns: exactly when results_of_chain reads it)
                    if (rc == PG_OK) out[s0 + s][names[c]] = results_of_chain(flat[c], cov.data(), goff[c], lik.data(), lexp.data());
                }
            if (rc != PG_OK) break;
        }
    } catch (...) {
        pg_job_destroy(job);
        throw;
    }
    pg_job_destroy(job);
    check_rc(rc, err);
    return out;
}

// ------------------------------------------------------------------ sampled cohort job
// a chain's picks as HaplotypeSampler::get_sampled_paths() has them (src/haplotypesampler.cpp:28-44)
static void sampled_paths_of(const uint32_t* picks, uint32_t size, size_t V, bool add_reference, SampledPaths* sampled) {
    for (uint32_t i = 0; i < size; ++i) sampled->sampled_paths.emplace_back(picks + (size_t)i * V, picks + (size_t)(i + 1) * V);
    if (add_reference) sampled->sampled_paths.push_back(std::vector<size_t>(V, 0));
}

// The fetch tail of one chain of a sampled cohort job (chain id = sample * n_contigs + contig), shared by
// genotype_cohort_sampled and genotype_cohort_sampled_reads: the reduced panel back from the device (the allele ids of the
// results are its own), the results over it, and the picks as HaplotypeSampler::get_sampled_paths() has them.  `full` = the
// contig over ALL paths; `coverage` = the chain's local coverages, or null: then they are what pg_job_fetch hands out (a
// chain whose counts never were on the host).  Returns the C ABI's code, its text in `err`.
static int fetch_sampled_chain(pg_job* job, uint32_t chain, const FlatContig& full, const uint16_t* coverage, uint32_t size, bool add_reference,
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
    const uint64_t n = goff.back();
    std::vector<double> lik(n ? n : 1);
    std::vector<int32_t> lexp(n ? n : 1);
    std::vector<uint16_t> cov(V ? V : 1);
    pg_contig_result res{};
    res.lik = lik.data(); res.lik_exp = lexp.data();
    if (!coverage) res.coverage = cov.data();
    rc = pg_job_fetch(job, chain, &res, err, errlen);
    if (rc != PG_OK) return rc;
    // (pg_job_fetch hands the coverage out only when the chain has columns: exactly when results_of_chain reads it)
    *results = results_of_chain(r, coverage ? coverage : cov.data(), goff, lik.data(), lexp.data());
    if (sampled) sampled_paths_of(picks, size, V, add_reference, sampled);
    return PG_OK;
}

std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_sampled(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::vector<SampleCounts>& samples,
    size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (sampled) sampled->assign(S, {});
    if (C == 0 || S == 0) return out;
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);   // ALL paths of the panel
    std::vector<pg_contig_batch> index(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        index[c] = flat[c].batch;
        c += 1;
    }
    static const uint16_t none = 0;
    std::vector<std::vector<const uint16_t*>> count_rows(S, std::vector<const uint16_t*>(C)), cov_rows(S, std::vector<const uint16_t*>(C));
    std::vector<pg_sample_counts> rows(S);
    for (size_t s = 0; s < S; ++s) {
        for (c = 0; c < C; ++c) {
            const auto k = samples[s].kmer_count.find(names[c]), v = samples[s].coverage.find(names[c]);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != flat[c].kmer_count.size() ||
                v->second.size() != flat[c].variant_pos.size())
                fail("genotype_cohort_sampled: sample " + std::to_string(s) + " does not fit the index on " + names[c]);
            count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        rows[s].kmer_count = count_rows[s].data();
        rows[s].coverage = cov_rows[s].data();
    }
    const uint32_t size = (uint32_t)panel_size;
    std::vector<std::vector<uint32_t>> picks(sampled ? S * C : 0);
    std::vector<uint32_t*> pick_rows(S * C, nullptr);
    for (size_t g = 0; g < picks.size(); ++g) {
        picks[g].assign((size_t)size * flat[g % C].variant_pos.size() + 1, 0);
        pick_rows[g] = picks[g].data();
    }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[1024] = {0};
    pg_job* job = nullptr;
    int rc = pg_sampler_cohort_new(device, (uint32_t)C, index.data(), (uint32_t)S, rows.data(), size, add_reference ? 1 : 0, recombrate,
                                   sampling_effective_N, allele_penalty, probabilities->handle(), &prm, sampled ? pick_rows.data() : nullptr,
                                   nullptr, &job, err, sizeof(err));
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
    if (rc != PG_OK) { if (job) pg_job_destroy(job); check_rc(rc, err); }
    for (size_t s = 0; s < S && rc == PG_OK; ++s)
        for (c = 0; c < C && rc == PG_OK; ++c)
            rc = fetch_sampled_chain(job, (uint32_t)(s * C + c), flat[c], cov_rows[s][c], size, add_reference, sampled ? picks[s * C + c].data() : nullptr,
                                     &out[s][names[c]], sampled ? &(*sampled)[s][names[c]] : nullptr, err, sizeof(err));
    pg_job_destroy(job);
    check_rc(rc, err);
    return out;
}

// ------------------------------------------------------------------ sampled cohort job fed by the device counter
std::vector<std::map<std::string, std::vector<GenotypingResult>>> genotype_cohort_sampled_reads(
    UniqueKmersMap& index, const std::string& prefix, const std::vector<std::string>& readfiles, const std::vector<size_t>& kmer_coverages,
    size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    auto& chromosomes = index.unique_kmers;
    const size_t C = chromosomes.size(), S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_sampled_reads: one k-mer coverage per read file");
    std::vector<std::map<std::string, std::vector<GenotypingResult>>> out(S);
    if (sampled) sampled->assign(S, {});
    if (C == 0 || S == 0) return out;
    const size_t B = std::max<size_t>(1, std::min(batch, S));
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    std::vector<std::string> names;
    std::vector<FlatContig> flat(C);   // ALL paths of the panel
    std::vector<pg_contig_batch> batches(C);
    std::vector<uint64_t> n_kmers(C);
    std::vector<uint32_t> n_variants(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {   // (map order: the plan's)
        names.push_back(kv.first);
        flatten(&kv.second, nullptr, flat[c]);
        batches[c] = flat[c].batch;
        n_kmers[c] = flat[c].kmer_count.size();
        n_variants[c] = (uint32_t)flat[c].variant_pos.size();
        c += 1;
    }
    const uint32_t size = (uint32_t)panel_size;
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[1024] = {0};
    auto check_batch = [&](int rc) {   // (a batch that does not fit: the caller's remedy is a smaller one, it is never split here)
        if (rc == PG_ERR_NOMEM) fail(std::string(err) + " (genotype_cohort_sampled_reads: lower `batch`)");
        check_rc(rc, err);
    };
    for (size_t s0 = 0; s0 < S; s0 += B) {
        const size_t n = std::min(B, S - s0);
        pg_sampler_counts* counts = nullptr;
        pg_job* job = nullptr;
        int rc = pg_sampler_counts_new(device, (uint32_t)C, n_kmers.data(), n_variants.data(), (uint32_t)n, &counts, err, sizeof(err));
        check_batch(rc);
        try {
            std::vector<pg_sample_counts> rows(n);
            for (size_t s = 0; s < n; ++s) {
                uint16_t* const* d_k = nullptr;
                uint16_t* const* d_c = nullptr;
                check_rc(pg_sampler_counts_rows(counts, (uint32_t)s, &d_k, &d_c, err, sizeof(err)), err);
                counter.reset_counts();
                counter.count(readfiles[s0 + s]);
                plan.fill_device(kmer_coverages[s0 + s], d_k, d_c);
                rows[s].kmer_count = d_k;
                rows[s].coverage = d_c;
            }
            std::vector<std::vector<uint32_t>> picks(sampled ? n * C : 0);
            std::vector<uint32_t*> pick_rows(n * C, nullptr);
            for (size_t g = 0; g < picks.size(); ++g) {
                picks[g].assign((size_t)size * flat[g % C].variant_pos.size() + 1, 0);
                pick_rows[g] = picks[g].data();
            }
            rc = pg_sampler_cohort_new_device(device, (uint32_t)C, batches.data(), (uint32_t)n, rows.data(), size, add_reference ? 1 : 0, recombrate,
                                              sampling_effective_N, allele_penalty, probabilities->handle(), &prm, sampled ? pick_rows.data() : nullptr,
                                              nullptr, &job, err, sizeof(err));
            pg_sampler_counts_destroy(counts);   // (the job does not reference the arrays)
            counts = nullptr;
            if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, sizeof(err));
            for (size_t s = 0; s < n && rc == PG_OK; ++s)
                for (c = 0; c < C && rc == PG_OK; ++c)
                    rc = fetch_sampled_chain(job, (uint32_t)(s * C + c), flat[c], nullptr, size, add_reference, sampled ? picks[s * C + c].data() : nullptr,
                                             &out[s0 + s][names[c]], sampled ? &(*sampled)[s0 + s][names[c]] : nullptr, err, sizeof(err));
        } catch (...) {
            if (counts) pg_sampler_counts_destroy(counts);
            if (job) pg_job_destroy(job);
            throw;
        }
        if (job) pg_job_destroy(job);
        check_batch(rc);
    }
    return out;
}

// ------------------------------------------------------------------ sampled cohort job, the sample column per VCF record
namespace {

// what the record tail needs of one chromosome: depends on the index alone, made once whatever the samples and batches
struct RecordChromosome {
    std::string name;
    const Graph* graph = nullptr;
    RecordPlan plan;
    std::vector<uint64_t> gl_off;
};

// refuses a missing graph or one whose bubble count is not the index's, as cohort_record_fields does; needs no device
std::vector<RecordChromosome> record_chromosomes(const std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes,
                                                 const std::map<std::string, Graph>& graphs, const char* who) {
    std::vector<RecordChromosome> out;
    for (const auto& kv : chromosomes) {
        const auto g = graphs.find(kv.first);
        if (g == graphs.end() || g->second.size() != kv.second.size()) fail(std::string(who) + ": no graph of " + kv.first + " with the index's bubbles");
        RecordChromosome rc;
        rc.name = kv.first;
        rc.graph = &g->second;
        rc.plan = g->second.record_plan();
        rc.gl_off.assign(rc.plan.nr_of_records() + 1, 0);
        const pg_record_plan view = rc.plan.view();
        if (pg_record_gl_offsets(&view, rc.gl_off.data()) != PG_OK) fail(std::string(who) + ": pg_record_gl_offsets refused the record plan of " + kv.first);
        out.push_back(std::move(rc));
    }
    return out;
}

// The tail of one sampled cohort job (made, not yet run; chains = n samples x C chromosomes, every chain its own index contig)
// behind pg_sampler_cohort_new[_device]: one strided plan per chromosome, the run, the record calls and GL values, the two
// packed fetches, and per chain the fields with what the device deferred finished from that chain's own reduced panel and
// bins (fetch_sampled_chain).  `cov_rows` = the samples' own coverages ([n][C]) or null: then what pg_job_fetch hands out.
// out[s] / sampled[s] (may be null) = sample s of this job.  Returns the C ABI's code, its text in `err`.
int sampled_job_record_fields(pg_job* job, size_t n, const std::vector<RecordChromosome>& chroms, const std::vector<FlatContig>& flat,
                              const std::vector<std::vector<const uint16_t*>>* cov_rows, uint32_t size, bool add_reference, bool ignore_imputed,
                              const std::vector<std::vector<uint32_t>>& picks, std::map<std::string, SampledRecordFields>* out,
                              std::map<std::string, SampledPaths>* sampled, char* err, size_t errlen, std::map<std::string, RecordText>* text = nullptr) {
    const size_t C = chroms.size();
    int rc = PG_OK;
    for (size_t c = 0; c < C && rc == PG_OK; ++c) {   // one plan per chromosome, checked and uploaded once for all samples
        const pg_record_plan view = chroms[c].plan.view();
        rc = pg_job_record_plan_strided(job, (uint32_t)c, (uint32_t)C, &view, err, errlen);
    }
    if (rc == PG_OK) rc = pg_job_run(job, nullptr, err, errlen);
    if (rc == PG_OK && text) {   // the column as bytes (genotype_cohort_sampled_record_text): one packed copy, then chain by chain
        std::vector<uint64_t> first, off;
        std::string packed;
        rc = job_record_text(job, n * C, ignore_imputed, &first, &off, &packed, err, errlen);
        for (size_t s = 0; s < n && rc == PG_OK; ++s)
            for (size_t c = 0; c < C && rc == PG_OK; ++c) {
                const uint32_t chain = (uint32_t)(s * C + c);
                const RecordChromosome& x = chroms[c];
                const size_t V = flat[c].variant_pos.size();
                if (first[chain + 1] - first[chain] != x.plan.nr_of_records()) {
                    std::snprintf(err, errlen, "genotype_cohort_sampled_record_text: chain %u holds other records than its plan's", chain);
                    return PG_ERR_INVALID;
                }
                std::vector<uint16_t> nk(V ? V : 1, 0), cov(V ? V : 1, 0);   // (by pg_job_fetch's rule; host memory of the job)
                pg_contig_result meta{};
                meta.n_kmers = nk.data(); meta.coverage = cov.data();
                rc = pg_job_fetch(job, chain, &meta, err, errlen);
                if (rc != PG_OK) break;
                const uint16_t* own = cov_rows ? (*cov_rows)[s][c] : nullptr;
                RecordText& t = text[s][x.name];
                t.unique_kmers.assign(nk.begin(), nk.begin() + V);
                if (sampled) sampled_paths_of(picks[chain].data(), size, V, add_reference, &sampled[s][x.name]);
                rc = chain_record_text(
                    job, chain, *x.graph, x.plan, x.gl_off, ignore_imputed, off.data() + first[chain], packed, [&](size_t v) { return t.unique_kmers[v] == 0; },
                    [&](size_t v) { return (uint16_t)(own && meta.n_columns > 0 ? own[v] : own ? 0 : cov[v]); },
                    [&](std::vector<GenotypingResult>* full) {
                        return fetch_sampled_chain(job, chain, flat[c], own, size, add_reference, nullptr, full, nullptr, err, errlen);
                    },
                    t, err, errlen);
            }
        return rc;
    }
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
            const RecordChromosome& x = chroms[c];
            const size_t V = flat[c].variant_pos.size();
            if (calls_first[chain + 1] - calls_first[chain] != x.plan.nr_of_records() || gl_first[chain + 1] - gl_first[chain] != x.gl_off.back()) {
                std::snprintf(err, errlen, "genotype_cohort_sampled_record_fields: chain %u holds other records than its plan's", chain);
                return PG_ERR_INVALID;
            }
            SampledRecordFields& f = out[s][x.name];
            // per bubble: the reduced panel's k-mer count and the coverage, by pg_job_fetch's rule (a chain without a kept
            // column reports neither); host memory of the job, no device copy
            std::vector<uint16_t> nk(V ? V : 1, 0), cov(V ? V : 1, 0);
            pg_contig_result meta{};
            meta.n_kmers = nk.data(); meta.coverage = cov.data();
            rc = pg_job_fetch(job, chain, &meta, err, errlen);
            if (rc != PG_OK) break;
            const uint16_t* own = cov_rows ? (*cov_rows)[s][c] : nullptr;
            f.unique_kmers.assign(nk.begin(), nk.begin() + V);
            f.coverage.resize(V);
            for (size_t v = 0; v < V; ++v) f.coverage[v] = own && meta.n_columns > 0 ? own[v] : own ? 0 : cov[v];
            f.fields.gl_off = x.gl_off;
            f.fields.gl.assign(gls.begin() + gl_first[chain], gls.begin() + gl_first[chain + 1]);
            const uint32_t* pk = sampled ? picks[chain].data() : nullptr;
            if (sampled) sampled_paths_of(pk, size, V, add_reference, &sampled[s][x.name]);
            rc = chain_record_fields(
                *x.graph, x.plan, recs.data() + calls_first[chain], ignore_imputed, true, [&](size_t v) { return f.unique_kmers[v] == 0; },
                [&](std::vector<GenotypingResult>* full) {
                    return fetch_sampled_chain(job, chain, flat[c], own, size, add_reference, nullptr, full, nullptr, err, errlen);
                },
                f.fields);
        }
    return rc;
}

}  // namespace

// genotype_cohort_sampled_record_fields and, with `text`, genotype_cohort_sampled_record_text: one sampled cohort job
static std::vector<std::map<std::string, SampledRecordFields>> sampled_cohort_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled, std::vector<std::map<std::string, RecordText>>* text) {
    const size_t C = chromosomes.size(), S = samples.size();
    std::vector<std::map<std::string, SampledRecordFields>> out(S);
    if (sampled) sampled->assign(S, {});
    if (text) text->assign(S, {});
    if (C == 0 || S == 0) return out;
    const std::vector<RecordChromosome> chroms = record_chromosomes(chromosomes, graphs, "genotype_cohort_sampled_record_fields");
    // (the job is made exactly as genotype_cohort_sampled makes it)
    std::vector<FlatContig> flat(C);   // ALL paths of the panel
    std::vector<pg_contig_batch> index(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {
        flatten(&kv.second, nullptr, flat[c]);
        index[c] = flat[c].batch;
        c += 1;
    }
    static const uint16_t none = 0;
    std::vector<std::vector<const uint16_t*>> count_rows(S, std::vector<const uint16_t*>(C)), cov_rows(S, std::vector<const uint16_t*>(C));
    std::vector<pg_sample_counts> rows(S);
    for (size_t s = 0; s < S; ++s) {
        for (c = 0; c < C; ++c) {
            const auto k = samples[s].kmer_count.find(chroms[c].name), v = samples[s].coverage.find(chroms[c].name);
            if (k == samples[s].kmer_count.end() || v == samples[s].coverage.end() || k->second.size() != flat[c].kmer_count.size() ||
                v->second.size() != flat[c].variant_pos.size())
                fail("genotype_cohort_sampled_record_fields: sample " + std::to_string(s) + " does not fit the index on " + chroms[c].name);
            count_rows[s][c] = k->second.empty() ? &none : k->second.data();
            cov_rows[s][c] = v->second.empty() ? &none : v->second.data();
        }
        rows[s].kmer_count = count_rows[s].data();
        rows[s].coverage = cov_rows[s].data();
    }
    const uint32_t size = (uint32_t)panel_size;
    std::vector<std::vector<uint32_t>> picks(sampled ? S * C : 0);
    std::vector<uint32_t*> pick_rows(S * C, nullptr);
    for (size_t g = 0; g < picks.size(); ++g) {
        picks[g].assign((size_t)size * flat[g % C].variant_pos.size() + 1, 0);
        pick_rows[g] = picks[g].data();
    }
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[1024] = {0};
    pg_job* job = nullptr;
    int rc = pg_sampler_cohort_new(device, (uint32_t)C, index.data(), (uint32_t)S, rows.data(), size, add_reference ? 1 : 0, recombrate,
                                   sampling_effective_N, allele_penalty, probabilities->handle(), &prm, sampled ? pick_rows.data() : nullptr,
                                   nullptr, &job, err, sizeof(err));
    try {
        if (rc == PG_OK)
            rc = sampled_job_record_fields(job, S, chroms, flat, &cov_rows, size, add_reference, ignore_imputed, picks, out.data(),
                                           sampled ? sampled->data() : nullptr, err, sizeof(err), text ? text->data() : nullptr);
    } catch (...) {
        if (job) pg_job_destroy(job);
        throw;
    }
    if (job) pg_job_destroy(job);
    check_rc(rc, err);
    return out;
}

std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_record_fields(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_cohort_record_fields(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities, recombrate,
                                        uniform, effective_N, device, ignore_imputed, sampled, nullptr);
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_record_text(
    std::map<std::string, std::vector<std::shared_ptr<UniqueKmers>>>& chromosomes, const std::map<std::string, Graph>& graphs,
    const std::vector<SampleCounts>& samples, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    std::vector<std::map<std::string, RecordText>> text;
    sampled_cohort_record_fields(chromosomes, graphs, samples, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities, recombrate,
                                 uniform, effective_N, device, ignore_imputed, sampled, &text);
    return text;
}

// genotype_cohort_sampled_reads_record_fields and, with `text`, genotype_cohort_sampled_reads_record_text: the same batches
static std::vector<std::map<std::string, SampledRecordFields>> sampled_reads_record_fields(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled, std::vector<std::map<std::string, RecordText>>* text) {
    auto& chromosomes = index.unique_kmers;
    const size_t C = chromosomes.size(), S = readfiles.size();
    if (kmer_coverages.size() != S) fail("genotype_cohort_sampled_reads_record_fields: one k-mer coverage per read file");
    std::vector<std::map<std::string, SampledRecordFields>> out(S);
    if (sampled) sampled->assign(S, {});
    if (text) text->assign(S, {});
    if (C == 0 || S == 0) return out;
    const std::vector<RecordChromosome> chroms = record_chromosomes(chromosomes, graphs, "genotype_cohort_sampled_reads_record_fields");
    // (counter, count plan and batches exactly as genotype_cohort_sampled_reads makes them)
    const size_t B = std::max<size_t>(1, std::min(batch, S));
    DeviceKmerCounter counter(index.kmersize, false, device);
    DeviceCountPlan plan(counter, index, prefix, true);
    std::vector<FlatContig> flat(C);   // ALL paths of the panel
    std::vector<pg_contig_batch> batches(C);
    std::vector<uint64_t> n_kmers(C);
    std::vector<uint32_t> n_variants(C);
    size_t c = 0;
    for (auto& kv : chromosomes) {   // (map order: the plan's)
        flatten(&kv.second, nullptr, flat[c]);
        batches[c] = flat[c].batch;
        n_kmers[c] = flat[c].kmer_count.size();
        n_variants[c] = (uint32_t)flat[c].variant_pos.size();
        c += 1;
    }
    const uint32_t size = (uint32_t)panel_size;
    pg_hmm_params prm{};
    prm.effective_N = effective_N; prm.recombrate = recombrate; prm.uniform = uniform ? 1 : 0; prm.run_genotyping = 1;
    char err[1024] = {0};
    auto check_batch = [&](int rc) {   // (a batch that does not fit: the caller's remedy is a smaller one, it is never split here)
        if (rc == PG_ERR_NOMEM) fail(std::string(err) + " (genotype_cohort_sampled_reads_record_fields: lower `batch`)");
        check_rc(rc, err);
    };
    for (size_t s0 = 0; s0 < S; s0 += B) {
        const size_t n = std::min(B, S - s0);
        pg_sampler_counts* counts = nullptr;
        pg_job* job = nullptr;
        int rc = pg_sampler_counts_new(device, (uint32_t)C, n_kmers.data(), n_variants.data(), (uint32_t)n, &counts, err, sizeof(err));
        check_batch(rc);
        try {
            std::vector<pg_sample_counts> rows(n);
            for (size_t s = 0; s < n; ++s) {
                uint16_t* const* d_k = nullptr;
                uint16_t* const* d_c = nullptr;
                check_rc(pg_sampler_counts_rows(counts, (uint32_t)s, &d_k, &d_c, err, sizeof(err)), err);
                counter.reset_counts();
                counter.count(readfiles[s0 + s]);
                plan.fill_device(kmer_coverages[s0 + s], d_k, d_c);
                rows[s].kmer_count = d_k;
                rows[s].coverage = d_c;
            }
            std::vector<std::vector<uint32_t>> picks(sampled ? n * C : 0);
            std::vector<uint32_t*> pick_rows(n * C, nullptr);
            for (size_t g = 0; g < picks.size(); ++g) {
                picks[g].assign((size_t)size * flat[g % C].variant_pos.size() + 1, 0);
                pick_rows[g] = picks[g].data();
            }
            rc = pg_sampler_cohort_new_device(device, (uint32_t)C, batches.data(), (uint32_t)n, rows.data(), size, add_reference ? 1 : 0, recombrate,
                                              sampling_effective_N, allele_penalty, probabilities->handle(), &prm, sampled ? pick_rows.data() : nullptr,
                                              nullptr, &job, err, sizeof(err));
            pg_sampler_counts_destroy(counts);   // (the job does not reference the arrays)
            counts = nullptr;
            if (rc == PG_OK)
                rc = sampled_job_record_fields(job, n, chroms, flat, nullptr, size, add_reference, ignore_imputed, picks, out.data() + s0,
                                               sampled ? sampled->data() + s0 : nullptr, err, sizeof(err), text ? text->data() + s0 : nullptr);
        } catch (...) {
            if (counts) pg_sampler_counts_destroy(counts);
            if (job) pg_job_destroy(job);
            throw;
        }
        if (job) pg_job_destroy(job);
        check_batch(rc);
    }
    return out;
}

std::vector<std::map<std::string, SampledRecordFields>> genotype_cohort_sampled_reads_record_fields(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    return sampled_reads_record_fields(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N,
                                       probabilities, recombrate, uniform, effective_N, device, batch, ignore_imputed, sampled, nullptr);
}

std::vector<std::map<std::string, RecordText>> genotype_cohort_sampled_reads_record_text(
    UniqueKmersMap& index, const std::map<std::string, Graph>& graphs, const std::string& prefix, const std::vector<std::string>& readfiles,
    const std::vector<size_t>& kmer_coverages, size_t panel_size, bool add_reference, unsigned short allele_penalty, long double sampling_effective_N,
    ProbabilityTable* probabilities, double recombrate, bool uniform, long double effective_N, int device, size_t batch, bool ignore_imputed,
    std::vector<std::map<std::string, SampledPaths>>* sampled) {
    std::vector<std::map<std::string, RecordText>> text;
    sampled_reads_record_fields(index, graphs, prefix, readfiles, kmer_coverages, panel_size, add_reference, allele_penalty, sampling_effective_N, probabilities,
                                recombrate, uniform, effective_N, device, batch, ignore_imputed, sampled, &text);
    return text;
}

void HMM::combine_likelihoods(HMM& other) {
    if (genotyping_result_.size() != other.genotyping_result_.size())
        fail("HMM::combine_likelihoods: HMMs to be combined must be of the same size.");
    for (size_t i = 0; i < genotyping_result_.size(); ++i) genotyping_result_[i].combine(other.genotyping_result_[i]);
}
void HMM::normalize() {
    for (auto& g : genotyping_result_) g.normalize();
}

// ------------------------------------------------------------------ haplotype sampling
std::vector<bool> SampledPaths::mask_indexes(size_t column_index, size_t max_index) {
    std::vector<bool> masked(max_index + 1, true);
    for (size_t i = 0; i < sampled_paths.size(); ++i) {
        if (column_index >= sampled_paths[i].size())
            throw std::runtime_error("HaplotypeSampler::SampledPaths::mask_indexes: column_index exceeds number of columns.");
        const size_t index = sampled_paths[i][column_index];
        if (index > max_index) throw std::runtime_error("HaplotypeSampler::SampledPaths::mask_indexes: observed index exceeds max_index.");
        masked[index] = false;
    }
    return masked;
}

bool SampledPaths::recombination(size_t column_index, size_t path_id) {
    if (path_id >= sampled_paths.size()) throw std::runtime_error("HaplotypeSampler::SampledPaths::recombination: path_id does not exist.");
    if (column_index >= sampled_paths[path_id].size())
        throw std::runtime_error("HaplotypeSampler::SampledPaths::recombination: column_id does not exist.");
    if (column_index > 0) return sampled_paths[path_id][column_index - 1] != sampled_paths[path_id][column_index];
    return false;
}

SamplingEmissions::SamplingEmissions(std::shared_ptr<UniqueKmers> uk) : default_penalty(25) {
    std::vector<std::shared_ptr<UniqueKmers>> one{uk};
    FlatContig f;
    std::vector<unsigned short> all;  // every path: the costs do not depend on the selection, but flatten needs one
    flatten(&one, nullptr, f);
    std::vector<uint16_t> cost(f.allele_id.size());
    if (pg_sampler_emission_costs(&f.batch, cost.data()) != PG_OK) throw std::runtime_error("SamplingEmissions: pg_sampler_emission_costs failed");
    unsigned short max_allele = 0;
    for (uint16_t a : f.allele_id) max_allele = std::max<unsigned short>(max_allele, a);
    allele_penalties.assign((size_t)max_allele + 1, 0);
    for (size_t s = 0; s < f.allele_id.size(); ++s) allele_penalties[f.allele_id[s]] = cost[s];
}

unsigned int SamplingEmissions::get_emission_cost(unsigned short allele_id) const { return allele_penalties.at(allele_id); }

void SamplingEmissions::penalize(unsigned short allele_id, unsigned short penalty) {
    allele_penalties.at(allele_id) += penalty;
    if (allele_penalties[allele_id] > default_penalty) allele_penalties[allele_id] = (unsigned short)default_penalty;
}

SamplingTransitions::SamplingTransitions(size_t from_variant, size_t to_variant, double recomb_rate, unsigned short nr_paths, long double effective_N)
    : cost(pg_sampler_transition_cost(from_variant, to_variant, recomb_rate, nr_paths, effective_N)) {}

unsigned int SamplingTransitions::compute_transition_cost(bool recombination) { return recombination ? cost : 0u; }

namespace {
thread_local int g_sampler_device = 0;
}
void HaplotypeSampler::set_device(int device) { g_sampler_device = device; }

HaplotypeSampler::HaplotypeSampler(std::vector<std::shared_ptr<UniqueKmers>>* uks, size_t size, double recombrate, long double effective_N,
                                   std::vector<unsigned int>* best_scores, bool add_reference, std::string path_output,
                                   std::string chromosome, unsigned short allele_penalty, double* time)
    : unique_kmers(uks) {
    const auto t0 = std::chrono::steady_clock::now();
    if (size < 1) return;
    const size_t V = uks->size();
    if (V > 0) {
        FlatContig f;
        flatten(uks, nullptr, f);  // ALL paths of the panel
        std::vector<uint32_t> sampled(size * V), best(size);
        char err[512] = {0};
        const int rc = pg_sampler_run(&f.batch, (uint32_t)size, recombrate, effective_N, allele_penalty, g_sampler_device, sampled.data(),
                                      best.data(), err, sizeof(err));
        if (rc != PG_OK) throw std::runtime_error(std::string("HaplotypeSampler: ") + err);
        for (size_t i = 0; i < size; ++i) {
            sampled_paths.sampled_paths.emplace_back(sampled.begin() + i * V, sampled.begin() + (i + 1) * V);
            if (best_scores != nullptr) best_scores->push_back(best[i]);
        }
    } else {
        for (size_t i = 0; i < size; ++i) sampled_paths.sampled_paths.emplace_back();
    }
    if (add_reference) sampled_paths.sampled_paths.push_back(std::vector<size_t>(V, 0));
    if (path_output != "") {  // reference src/haplotypesampler.cpp:46-66
        std::ofstream out(path_output);
        out << "#chromosome\tposition";
        for (size_t p = 0; p < sampled_paths.sampled_paths.size(); ++p) out << "\tHaplotypeID_path" << p << "\tRecombination_path" << p;
        out << std::endl;
        for (size_t c = 0; c < V; ++c) {
            out << chromosome << "\t" << uks->at(c)->get_variant_position();
            for (size_t p = 0; p < sampled_paths.sampled_paths.size(); ++p)
                out << "\t" << sampled_paths.sampled_paths[p][c] << "\t" << sampled_paths.recombination(c, p);
            out << std::endl;
        }
    }
    update_unique_kmers();
    if (time != nullptr) *time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void HaplotypeSampler::get_column_minima(std::vector<unsigned int>& column, std::vector<bool>& mask, size_t& first_id, size_t& second_id,
                                         unsigned int& first_val, unsigned int& second_val) const {
    std::vector<uint8_t> m(mask.begin(), mask.end());
    uint32_t out4[4];
    char err[256] = {0};
    if (pg_sampler_column_minima(column.data(), m.data(), (uint32_t)column.size(), g_sampler_device, out4, err, sizeof(err)) != PG_OK)
        throw std::runtime_error(std::string("HaplotypeSampler::get_column_minima: ") + err);
    // absent entries: numeric_limits<unsigned int>::max() widened to size_t, as in the reference
    first_id = out4[0]; second_id = out4[1]; first_val = out4[2]; second_val = out4[3];
}

void HaplotypeSampler::update_unique_kmers() {
    const size_t nr_paths = sampled_paths.sampled_paths.size();
    for (size_t i = 0; i < unique_kmers->size(); ++i) {
        std::vector<unsigned short> p(nr_paths);
        for (size_t j = 0; j < nr_paths; ++j) p[j] = (unsigned short)sampled_paths.sampled_paths[j][i];
        (*unique_kmers)[i]->update_paths(p);
    }
}

}  // namespace pangenie
