"""The unit entry points of the phasing column on the device (pg_record_phase_from_haplotypes, pg_phase_text_from_fields; k_rphase
and k_ptext_* of pangenie_amd/csrc/pg_phase_text.hip) against the Python mirror of the rule (tests/phase_util.py): the exhaustive
format set in one launch; record counts at one record, one short of a block, a block, one more and five blocks, with a guard
region behind the offsets and behind the text left untouched; and the decisions on constructed plans — bubbles of several
records, a haplotype on an undefined allele of one record and a defined allele of its sibling, records with undefined alleles
with and without stored likelihoods."""
import numpy as np
import pytest

from pangenie_amd import _lib, calls
from tests.phase_util import BOUND, UNDEFINED, as_pairs, mirror_phase, mirror_text

pytestmark = pytest.mark.gpu
ALLELES = [0, 1, 9, 10, 99, 100, 255, UNDEFINED]
KCS = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]


def phase_array(pairs):
    ph = np.zeros(len(pairs), calls.PHASE_DTYPE)
    if len(pairs):
        ph["allele_1"], ph["allele_2"] = np.asarray(pairs)[:, 0], np.asarray(pairs)[:, 1]
    return ph


def test_the_exhaustive_format_set_in_one_launch():
    rows = [(a1, a2, kc, nc) for a1 in ALLELES for a2 in ALLELES for kc in KCS for nc in (0, 1)]
    pairs = np.array([(r[0], r[1]) for r in rows], np.int64)
    kc, nc = np.array([r[2] for r in rows], np.uint16), np.array([r[3] for r in rows], np.uint8)
    off, text = calls.phase_text_from_fields(phase_array(pairs), kc, nc)
    want_off, want = mirror_text(pairs, kc, nc)
    assert off.astype(np.int64).tolist() == want_off.tolist() and text == want
    assert np.diff(want_off).max() == BOUND   # (reached, never exceeded)
    at = rows.index((255, 255, 65535, 0))
    assert text[int(off[at]):int(off[at + 1])] == b"255|255:65535"
    # without the no_call array nothing is a no-call
    off2, text2 = calls.phase_text_from_fields(phase_array(pairs), kc)
    want_off2, want2 = mirror_text(pairs, kc)
    assert off2.astype(np.int64).tolist() == want_off2.tolist() and text2 == want2
    assert b"./." not in text2 and b"./." in text


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1025])
def test_record_counts_around_the_block_and_the_guard_regions(R):
    rng = np.random.default_rng(5100 + R)
    pairs = rng.choice(ALLELES, (R, 2))
    kc = rng.choice(KCS + [65535] * 3, R).astype(np.uint16)
    nc = (rng.random(R) < 0.2).astype(np.uint8)
    if R >= 256:   # one whole block at the bound: its stage is full to the last byte
        pairs[:256], kc[:256], nc[:256] = 255, 65535, 0
    ph = phase_array(pairs)
    want_off, want = mirror_text(pairs, kc, nc)
    lib, cap, guard = _lib.load_hip(), calls.phase_text_bound(R), 64
    off = np.full(R + 1 + guard, 0xA5A5A5A5A5A5A5A5, np.uint64)
    text = np.full(cap + guard, 0x23, np.uint8)
    rc = lib.pg_phase_text_from_fields(0, R, ph.ctypes.data, kc.ctypes.data, nc.ctypes.data, off.ctypes.data, text.ctypes.data, cap)
    assert rc == 0
    assert off[:R + 1].astype(np.int64).tolist() == want_off.tolist() and text[:len(want)].tobytes() == want
    assert (off[R + 1:] == 0xA5A5A5A5A5A5A5A5).all() and (text[len(want):] == 0x23).all()
    if R >= 256:
        assert int(off[256]) == 256 * BOUND


def constructed():
    """bubble 0: one record, all defined; bubble 1: two records over five bubble alleles, the first with an undefined allele that
    bubble allele 3 carries while the second record's allele of bubble allele 3 is defined; bubble 2: three records, one without
    undefined alleles; bubble 3: one record whose only ALT is undefined"""
    bubbles = [
        [([0, 1], [True, True])],
        [([0, 1, 1, 2, 0], [True, True, False]), ([0, 0, 1, 1, 2], [True, True, True])],
        [([0, 1, 2, 3], [True, False, True, True]), ([0, 0, 1, 1], [True, True]), ([0, 1, 0, 2], [True, True, False])],
        [([0, 1], [True, False])],
    ]
    return calls.RecordPlan.from_records(bubbles)


@pytest.mark.parametrize("keyed", [(1, 1, 1, 1), (0, 0, 0, 0), (1, 0, 1, 0)])
def test_decisions_on_constructed_plans(keyed):
    plan = constructed()
    keyed = np.array(keyed, np.uint8)
    for h1, h2 in (([1, 3, 2, 1], [0, 1, 3, 0]), ([0, 4, 1, 0], [1, 3, 0, 1]), ([1, 2, 3, 1], [1, 2, 3, 1])):
        got = as_pairs(calls.record_phase_from_haplotypes(plan, np.array(h1, np.uint16), np.array(h2, np.uint16), keyed))
        want = mirror_phase(plan, h1, h2, keyed)
        assert got.tolist() == want.tolist(), (h1, h2, keyed.tolist())
    # spelled out for the first pair of haplotypes: bubble 1's haplotype 1 is on the undefined allele of record 1 and on
    # allele 1 of record 2 (all defined: never the quirk); bubble 2's records 1 and 3 have undefined alleles
    got = as_pairs(calls.record_phase_from_haplotypes(plan, np.array([1, 3, 2, 1], np.uint16), np.array([0, 1, 3, 0], np.uint16), keyed)).tolist()
    assert got[0] == [1, 0]
    assert got[1] == [UNDEFINED, 1 if keyed[1] else 0] and got[2] == [1, 0]
    assert got[3] == ([1, 2] if keyed[2] else [0, 0]) and got[4] == [1, 1] and got[5] == [0, UNDEFINED]
    assert got[6] == [UNDEFINED, 0]


def test_many_bubbles_over_several_blocks():
    rng = np.random.default_rng(5200)
    bubbles = []
    for _ in range(700):   # 1 .. 3 records each: more than five blocks of records
        n_ids = int(rng.integers(2, 9))
        records = []
        for _ in range(int(rng.integers(1, 4))):
            nA = int(rng.integers(2, min(n_ids, 6) + 1))
            own = rng.integers(0, nA, n_ids)
            own[0] = 0
            records.append((own.tolist(), [True] + [bool(x) for x in rng.random(nA - 1) >= 0.3]))
        bubbles.append((n_ids, records))
    plan = calls.RecordPlan.from_records([r for _, r in bubbles])
    h1 = np.array([rng.integers(0, n) for n, _ in bubbles], np.uint16)
    h2 = np.array([rng.integers(0, n) for n, _ in bubbles], np.uint16)
    keyed = (rng.random(len(bubbles)) < 0.5).astype(np.uint8)
    assert plan.n_records > 1280
    got = as_pairs(calls.record_phase_from_haplotypes(plan, h1, h2, keyed))
    want = mirror_phase(plan, h1, h2, keyed)
    assert got.tolist() == want.tolist()
    assert (want == UNDEFINED).any() and (want[:, 0] > 1).any()
