"""CPU: the latency histogram on the host.  The numpy mirror (upe_amd/latency.py),
upe_latency_record_batch and per-sample upe_latency_record agree word for word with the
reference's latency_record called once per sampled packet — or, without the reference, with the
results it gave when tests/golden/latency_cases.npz was written.  Percentile and merge against the
reference's, the refused calibrations, and saturation (where the reference is undefined: against
the mirror and by hand)."""
from __future__ import annotations

import numpy as np
import pytest

import latency_cases
import latency_ref
import oracle
from upe_amd import gpu, latency

CASES = latency_cases.cases()
DEFINED = [c for c in CASES if c.ref_defined]
UNDEFINED = [c for c in CASES if not c.ref_defined]
GOLD = latency_ref.load_golden()
M64 = 2**64 - 1


def _want(c):
    """The reference's histogram and percentiles for a case: computed where the reference is
    built, recorded otherwise."""
    if oracle.ref_available():
        h = latency_ref.ref_record(c)
        return h, latency_ref.ref_percentiles(h)
    _, h, pct = GOLD[c.name]
    return h, pct


def _c_batch(c, start=None):
    h = gpu.latency_init() if start is None else np.array(start, np.uint64)
    gpu.latency_record_batch(h, c.ts, c.verdicts, c.now, c.cpn)
    return h


def _c_samples(c):
    h = gpu.latency_init()
    take = latency.sampled(c.ts, c.verdicts)
    for t in c.ts[take].tolist():
        gpu.latency_record(h, (c.now - t) & M64, c.cpn)
    return h


def test_cases_cover_what_they_are_for():
    by = {c.name: c for c in CASES}
    assert len(DEFINED) >= 20 and len(UNDEFINED) >= 4
    h = latency_cases.expected(by["wrapped_subtraction"])
    assert int(h[latency.MAX]) == 2**63 and int(h[latency.TOTAL]) == 4
    assert int(h[latency.SUM]) < 2**63          # three samples of about 2^63: the sum wrapped
    h = latency_cases.expected(by["all_timestamps_zero"])
    assert h.tolist() == [0] * 9 + [1000000, 0, 0]
    assert latency_cases.expected(by["all_consumed"]).tolist() == latency.init().tolist()
    h = latency_cases.expected(by["one_bucket"])
    assert int(h[1]) == int(h[latency.TOTAL]) == 1500
    h = latency_cases.expected(by["all_above_1ms"])
    assert int(h[7]) == 700 and int(h[latency.MIN]) == 1000000
    h = latency_cases.expected(by["mixed_verdicts"])
    assert all(int(x) > 0 for x in h[:8]), "the sized cases reach every bucket"
    assert 0 < int(h[latency.TOTAL]) < int(latency_cases.expected(by["no_verdicts"])[latency.TOTAL])
    v = by["mixed_verdicts"].verdicts
    for g in range(0, 960, 64):
        assert set((v[g:g + 64] & 0xF).tolist()) == set(range(7))
    for cpn in latency_cases.CPNS:               # each bound is crossed inside its +-3 window
        ns = latency.to_ns(np.array(latency_cases.bound_cycles(cpn), np.uint64), cpn).reshape(8, 7)
        for b, row in zip(latency.BOUNDS, ns.tolist()):
            assert min(row) < b <= max(row), (cpn, b, row)
    # above 2^53 the conversion rounds: the mirror differs from exact integer division there
    big = by["above_2_53_cpn_1"]
    cyc = [(big.now - t) & M64 for t in big.ts.tolist()]
    assert latency.to_ns(np.array(cyc, np.uint64), 1.0).tolist() != cyc


@pytest.mark.parametrize("c", DEFINED, ids=lambda c: c.name)
def test_host_paths_match_the_reference(c):
    want, pct = _want(c)
    assert latency_cases.expected(c).tolist() == want.tolist(), "numpy mirror"
    assert _c_batch(c).tolist() == want.tolist(), "upe_latency_record_batch"
    assert _c_samples(c).tolist() == want.tolist(), "upe_latency_record per sample"
    for p, w in zip(latency_cases.PERCENTILES, pct.tolist()):
        assert latency.percentile(want, p) == w, f"mirror percentile {p}"
        assert gpu.latency_percentile(want, p) == w, f"upe_latency_percentile {p}"


def test_golden_holds_every_defined_case():
    assert sorted(GOLD) == sorted(c.name for c in DEFINED)
    for c in DEFINED:
        g = GOLD[c.name][0]
        assert np.array_equal(g.ts, c.ts) and g.now == c.now and g.cpn == c.cpn
        assert (g.verdicts is None) == (c.verdicts is None)
        assert c.verdicts is None or np.array_equal(g.verdicts, c.verdicts)


@pytest.mark.skipif(not oracle.ref_available(), reason="needs the reference build")
def test_golden_regenerates_identically():
    z = np.load(latency_ref.GOLDEN)
    new = latency_ref.build_golden()
    assert sorted(z.files) == sorted(new)
    for k in z.files:
        assert z[k].dtype == new[k].dtype and np.array_equal(z[k], new[k]), k


def test_init_and_empty_percentile():
    h = gpu.latency_init()
    assert h.tolist() == latency.init().tolist() == [0] * 9 + [1000000, 0, 0]
    if oracle.ref_available():
        assert latency_ref.ref_init().tolist() == h.tolist()
    for p in latency_cases.PERCENTILES:
        assert gpu.latency_percentile(h, p) == latency.percentile(h, p) == 0


def test_percentile_walks_the_buckets():
    """Hand-made histograms: the bound returned is the first bucket at which the cumulative count
    reaches (uint64)(p * total)."""
    h = latency.init()
    h[:8] = [10, 0, 30, 0, 0, 50, 9, 1]
    h[latency.TOTAL] = 100
    want = {0.0: 100, 0.05: 100, 0.1: 100, 0.11: 1000, 0.4: 1000, 0.41: 50000, 0.9: 50000,
            0.95: 100000, 0.99: 100000, 0.999: 100000, 1.0: 1000000}
    for p, w in want.items():
        assert gpu.latency_percentile(h, p) == latency.percentile(h, p) == w, p
        if oracle.ref_available():
            assert int(latency_ref.lib().latency_percentile(latency_ref._p(h), p)) == w
    # where the reference's cast is undefined: a negative or NaN percentile counts as 0
    for p in (-0.5, float("nan")):
        assert gpu.latency_percentile(h, p) == latency.percentile(h, p) == 100


def test_merge():
    hs = [_want(c)[0] for c in DEFINED]
    for a, b, ca, cb in zip(hs, hs[1:] + hs[:1], DEFINED, DEFINED[1:] + DEFINED[:1]):
        m = np.array(a, np.uint64)
        gpu.latency_merge(m, b)
        assert m.tolist() == latency.merge(a, b).tolist()
        # merging equals recording one case after the other into one histogram
        assert m.tolist() == _c_batch(cb, start=a).tolist() == \
            latency_cases.expected(cb, start=a).tolist()
        if oracle.ref_available():
            assert m.tolist() == latency_ref.ref_merge(a, b).tolist()
    e = gpu.latency_init()
    gpu.latency_merge(e, latency.init())
    assert e.tolist() == latency.init().tolist()


@pytest.mark.parametrize("cpn", [0.0, -0.0, -2.4, float("nan"), float("inf"), float("-inf")])
def test_refused_calibrations(cpn):
    c = latency_cases.sized(100)
    start = latency_cases.expected(c)
    h = start.copy()
    with pytest.raises(gpu.UpeGpuError) as e:
        gpu.latency_record(h, 1234, cpn)
    assert "cycles_per_ns" in str(e.value)
    with pytest.raises(gpu.UpeGpuError):
        gpu.latency_record_batch(h, c.ts, c.verdicts, c.now, cpn)
    assert h.tolist() == start.tolist(), "a refused call changed the histogram"
    with pytest.raises(ValueError):
        latency.record_host(h, c.ts, c.verdicts, c.now, cpn)
    assert not latency.cpn_ok(cpn)


def test_batch_argument_errors():
    h = gpu.latency_init()
    assert gpu.LIB.upe_latency_record_batch(gpu._np_ptr(h), None, None, 5, 1, 2.0) == -1
    assert gpu.LIB.upe_latency_record_batch(None, None, None, 0, 1, 2.0) == -1
    assert gpu.LIB.upe_latency_record(None, 1, 2.0) == -1
    assert gpu.LIB.upe_latency_record_batch(gpu._np_ptr(h), None, None, 0, 1, 2.0) == 0
    assert h.tolist() == latency.init().tolist()


@pytest.mark.parametrize("c", UNDEFINED, ids=lambda c: c.name)
def test_saturation(c):
    want = latency_cases.expected(c)
    assert int(want[latency.MAX]) == M64, "the case saturates"
    assert _c_batch(c).tolist() == want.tolist()
    assert _c_samples(c).tolist() == want.tolist()


def test_saturation_by_hand():
    """cycles / cpn of 2^64 or more gives UINT64_MAX; just below, the exact truncation."""
    h = gpu.latency_init()
    gpu.latency_record(h, M64, 1.0)              # (double)(2^64 - 1) = 2^64
    gpu.latency_record(h, 2**64 - 1025, 1.0)     # rounds down to 2^64 - 2048
    gpu.latency_record(h, 3, 1e-300)
    assert h.tolist() == [0] * 7 + [3, 3, 1000000, M64, (M64 + 2**64 - 2048 + M64) & M64]
    m = latency.init()
    for cyc, cpn in ((M64, 1.0), (2**64 - 1025, 1.0), (3, 1e-300)):
        m = latency.record_host(m, np.array([1], np.uint64), None, cyc + 1, cpn)
    assert m.tolist() == h.tolist()
