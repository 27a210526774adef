"""The count plan with 64-bit slot indices (kk_plan_resolve<uint64_t>, kk_plan_fill<uint64_t>: what a table of 2^32 slots or
more runs) on tables of test size: PG_COUNT_PLAN=wide, read when a plan is created.  The bodies are those of
tests/test_counts_gpu.py; every plan here is a pair, a wide and a narrow one over the same counter and lists, and every array
the wide one fills must equal the narrow one's as well as the restated host loop."""
import numpy as np
import pytest

from pangenie_amd import kmers
from tests import test_counts_gpu as narrow_tests
from tests.test_counts_gpu import assert_same, on_host

pytestmark = pytest.mark.gpu


class WideAndNarrow:
    """a wide plan with a narrow one beside it; answers the wide plan's results after comparing the two"""

    def __init__(self, monkeypatch, counter, contigs, lenient=False, short_lists=False):
        self.narrow = None
        monkeypatch.setenv("PG_COUNT_PLAN", "wide")
        try:
            self.wide = kmers.CountPlan(counter, contigs, lenient)   # (first: an error a test expects is the wide plan's)
        finally:
            monkeypatch.delenv("PG_COUNT_PLAN")
        self.narrow = kmers.CountPlan(counter, contigs, lenient)
        w, n = self.wide.stats(), self.narrow.stats()
        assert w[:3] == n[:3]
        codes = w.n_kmers + w.n_flanks
        # the switch is alive: 8 bytes an index against 4, everything else the same
        assert w.device_bytes >= 8 * codes and w.device_bytes - n.device_bytes == 4 * codes and codes > 0
        if not short_lists:   # (4 bytes a code plus the offsets and descriptors stay below 8 a code once the lists are longer than those)
            assert n.device_bytes < 8 * codes, (n.device_bytes, codes)
        self._h = self.wide._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.wide.close()
        if self.narrow is not None:
            self.narrow.close()

    def stats(self):
        return self.wide.stats()

    def last_fill_ms(self):
        return self.wide.last_fill_ms()

    def fill(self, kmer_coverage):
        got, same = self.wide.fill(kmer_coverage), self.narrow.fill(kmer_coverage)
        assert_same(got[0], same[0], f"wide against narrow, kmer_count at {kmer_coverage}")
        assert_same(got[1], same[1], f"wide against narrow, coverage at {kmer_coverage}")
        return got

    def fill_device(self, kmer_coverage):
        got, same = self.wide.fill_device(kmer_coverage), self.narrow.fill_device(kmer_coverage)
        assert_same(on_host(got[0]), on_host(same[0]), f"wide against narrow on the device, kmer_count at {kmer_coverage}")
        assert_same(on_host(got[1]), on_host(same[1]), f"wide against narrow on the device, coverage at {kmer_coverage}")
        return got

    def fill_job(self, job, sample, kmer_coverage):
        self.wide.fill_job(job, sample, kmer_coverage)   # (the narrow plan's arrays: fill() beside every fill_job of the body)


@pytest.fixture
def pair(monkeypatch):
    monkeypatch.delenv("PG_COUNT_PLAN", raising=False)
    return lambda counter, contigs, lenient=False: WideAndNarrow(monkeypatch, counter, contigs, lenient)


@pytest.mark.parametrize("k", [21, 32])
def test_wide_fill_equals_the_restated_host_loop(k, pair):
    """ragged, empty, no flanks, 700 variants, no unique k-mers; all of COVERAGES"""
    narrow_tests.fill_equals_the_restated_host_loop(k, pair)


def test_wide_named_cases_by_hand(monkeypatch):
    monkeypatch.delenv("PG_COUNT_PLAN", raising=False)
    # 12 codes: the 7 offsets and 2 descriptors of this plan alone are more than 8 bytes a code
    narrow_tests.named_cases_by_hand(lambda counter, contigs: WideAndNarrow(monkeypatch, counter, contigs, short_lists=True))


def test_wide_strict_plan_names_the_first_unregistered_code_and_a_lenient_one_counts_zero(pair):
    narrow_tests.strict_plan_names_the_first_unregistered_code_and_a_lenient_one_counts_zero(pair)


def test_wide_fill_job_equals_an_upload_of_the_host_filled_arrays(pair):
    narrow_tests.fill_job_equals_an_upload_of_the_host_filled_arrays(16, pair)


def test_any_other_value_of_the_switch_is_a_narrow_plan(monkeypatch):
    k = 21
    rng = np.random.default_rng(21)
    pool = np.unique(kmers.canonical_codes(narrow_tests.windows(narrow_tests.genome(rng, 900), k), k))
    contigs = [narrow_tests.contig_of(rng, pool, 80, 6, 20)]
    sizes = {}
    with kmers.KmerCounter(k) as counter:
        counter.add_codes(pool)
        for value in (None, "", "narrow", "WIDE", "wide"):
            if value is None:
                monkeypatch.delenv("PG_COUNT_PLAN", raising=False)
            else:
                monkeypatch.setenv("PG_COUNT_PLAN", value)
            with kmers.CountPlan(counter, contigs) as plan:
                sizes[value] = plan.stats().device_bytes
        monkeypatch.delenv("PG_COUNT_PLAN")
    n = contigs[0].kmer_code.size + contigs[0].flank_code.size
    assert sizes[None] == sizes[""] == sizes["narrow"] == sizes["WIDE"] == sizes["wide"] - 4 * n < 8 * n <= sizes["wide"]
