"""pg_gl_text and pg_record_gl_offsets (host only, no device): the text of a GL value is what `ostream << setprecision(4)`
gives of the long double logarithm — "%.4g" of the decimal the value holds: exponent and fixed notation, stripped zeros, "0",
"-inf", a positive value; formed here from np.longdouble logarithms by numpy's exact expansion.  The offsets follow the
defined alleles of every record, in the VCF's order of genotypes; a plan the library refuses is refused here."""
import ctypes as C

import numpy as np
import pytest

from pangenie_amd import _lib, build, calls

LD = np.longdouble


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return _lib.load_hip()


def value_of(v):
    """the (mant, exp10) of a long double logarithm: its four significant digits, from the exact expansion"""
    sci = np.format_float_scientific(LD(v), precision=3, unique=False, trim="k")
    mant, exp = sci.split("e")
    return int(mant.replace(".", "")), int(exp)


def test_text_is_what_setprecision_4_prints(lib):
    rng = np.random.default_rng(20261020)
    logs = [-LD(10) ** LD(rng.uniform(-20, 3.69)) for _ in range(4000)]            # every notation and magnitude a likelihood's log10 has
    logs += [LD(x) for x in ("-1000", "-4907", "-12", "-0.5", "-0.301", "-0.0001", "-0.00012", "-0.00001", "-1.5e-5", "-2.354e-20", "4.709e-20",
                             "-9.9996", "-99995", "-0.30102999566", "-3", "-30", "-300", "-0.03", "-100.04")]
    seen = set()
    for v in logs:
        mant, exp = value_of(v)
        want = "%.4g" % float(np.format_float_scientific(v, precision=3, unique=False, trim="k"))
        assert calls.gl_text((mant, exp)) == want, (v, mant, exp)
        seen.add("e" in want)
        seen.add("." in want)
    assert seen == {True, False}
    # stated, so that a formatter and a yardstick that agree on something else do not pass
    for (mant, exp), want in {(-1000, 3): "-1000", (-4907, 3): "-4907", (-1200, 1): "-12", (-5000, -1): "-0.5", (-3010, -1): "-0.301",
                              (-1000, -4): "-0.0001", (-1200, -4): "-0.00012", (-1000, -5): "-1e-05", (-1500, -5): "-1.5e-05",
                              (-2354, -20): "-2.354e-20", (4709, -20): "4.709e-20", (-1234, 0): "-1.234", (-1230, 2): "-123"}.items():
        assert calls.gl_text((mant, exp)) == want, (mant, exp)
    assert calls.gl_text((0, 0)) == "0" and calls.gl_text((0, calls.PG_GL_NEG_INF)) == "-inf"
    assert calls.gl_text((0, calls.PG_GL_DEFERRED)) is None and calls.gl_text((0, 5)) is None and calls.gl_text((999, 0)) is None
    # a buffer too small is refused, not overrun
    buf = C.create_string_buffer(4)
    assert lib.pg_gl_text(_lib.PgGl(-1234, 0), buf, 4) == -1 and lib.pg_gl_text(_lib.PgGl(-1200, 1), buf, 4) == 3 and buf.value == b"-12"
    assert lib.pg_gl_text(_lib.PgGl(-1234, 0), None, 0) == -1


def test_offsets_follow_the_defined_alleles_in_the_vcfs_order(lib):
    plan = calls.RecordPlan.from_records([
        [([0, 1, 2], [True, True, True]), ([0, 1, 1], [True, False])],     # 6 values, 1 value
        [([0], [True])],                                                    # 1
        [([0, 3, 2, 1], [True, False, True, True, False, True])],           # four defined of six: 10
    ])
    off = calls.record_gl_offsets(plan)
    assert off.dtype == np.uint64 and off.tolist() == [0, 6, 7, 8, 18]
    assert calls.record_gl_offsets(calls.RecordPlan.from_records([])).tolist() == [0]
    # refusals: null arguments, and what pg_job_record_plan refuses
    out = np.zeros(8, np.uint64)
    c = plan.as_c()
    assert lib.pg_record_gl_offsets(None, out.ctypes.data_as(_lib.u64p)) == _lib.PG_ERR_INVALID
    assert lib.pg_record_gl_offsets(C.addressof(c), None) == _lib.PG_ERR_INVALID
    bad = calls.RecordPlan.from_records([[([0, 1], [True, True])]])
    bad.vcf_index[1] = 5   # not the running count of defined alleles
    with pytest.raises(Exception) as e:
        calls.record_gl_offsets(bad)
    assert e.value.code == _lib.PG_ERR_INVALID
    bad = calls.RecordPlan.from_records([[([0, 2], [True, True])]])   # a map entry that is no allele of the record
    with pytest.raises(Exception) as e:
        calls.record_gl_offsets(bad)
    assert e.value.code == _lib.PG_ERR_INVALID
    wide = calls.RecordPlan.from_records([[([0], [True] * 257)]])
    with pytest.raises(Exception) as e:
        calls.record_gl_offsets(wide)
    assert e.value.code == _lib.PG_ERR_UNSUPPORTED
