"""upe_gpu_process_segmented and upe_gpu_process_segmented_resident on the chosen batches of
tests/segment_cases.py (pinned on the CPU by tests/test_segment_cases.py): the two calls against
each other and against the restated worker run segment by segment, bit for bit — whole verdict
words (UPE_VF_L1_INIT included: it is relative to each segment's start, and the oracle run is cut
where the case says the batch is cut), frames, counters, rule_stats, L1, the slot arrays field by
field — the info record against the case's stated numbers, and the snapshot the resident call
leaves loaded against the host arrays it returns.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import golden_io
import neigh_cases as nc
import oracle
import patch_cases as pc
import resolve_cases as rc
import segment_cases as sc
from test_gpu_latency import _hip
from test_gpu_parity import _assert_same
from test_gpu_resolve import gpu_resolve
from test_gpu_rule_tables import _set_mode
from upe_amd import gpu, neigh
from upe_amd.layout import CW_NDP

pytestmark = pytest.mark.gpu

NOW = sc.NOW
FIELDS = ["ip", "mac", "valid", "update_at"]
CALLS = ("segmented", "resident")


def _ref(r):
    return {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
            "rule_stats": r.rule_stats, "l1": r.l1}


class Dev:
    """A case's batch in device memory; stream: uploaded on it, nothing waited for."""

    def __init__(self, w, wl, stream=None):
        self.w, self.n = w, wl.n
        self.host = (np.ascontiguousarray(wl.frames), np.ascontiguousarray(wl.desc))
        self.frames = w.malloc(self.host[0].nbytes)
        self.desc = w.malloc(self.host[1].nbytes)
        self.verdict = w.malloc(4 * self.n)
        w.h2d(self.frames, self.host[0], stream=stream)
        w.h2d(self.desc, self.host[1], stream=stream)
        if not stream:
            w.sync()

    def fetch(self):
        """(frames, verdict), fetched on the context's stream and freed."""
        frames = np.empty(self.host[0].nbytes, np.uint8)
        verdict = np.empty(self.n, np.uint32)
        self.w.d2h(frames, self.frames)
        self.w.d2h(verdict, self.verdict)
        self.w.sync()
        for p in (self.frames, self.desc, self.verdict):
            self.w.free(p)
        return frames, verdict


def call(w, which, wl, arp, ndp, stream=None):
    """One call on worker w over the host arrays (updated in place): (outputs, (writes,) or
    (ctrl, writes, patched, rebuilds))."""
    b = Dev(w, wl, stream)
    if which == "segmented":
        info = (w.process_segmented(b.frames, b.desc, b.verdict, b.n, arp, ndp, now=NOW,
                                    stream=stream),)
    else:
        i = w.process_segmented_resident(b.frames, b.desc, b.verdict, b.n, arp, ndp, now=NOW,
                                         stream=stream)
        info = tuple(int(i[k]) for k in ("ctrl", "writes", "patched", "rebuilds"))
    frames, verdict = b.fetch()
    counters, stats = w.get_stats()
    return (frames, verdict, counters, stats, w.get_l1()), info


def check(got, info, arp, ndp, c, r, what, expect=None):
    """A call's outputs against the oracle run r and the case's stated numbers."""
    expect = c.expect if expect is None else expect
    _assert_same(got, _ref(r), what)
    for f in FIELDS[:3]:
        assert np.array_equal(arp[f], r.arp[f]) and np.array_equal(ndp[f], r.ndp[f]), (what, f)
    if len(info) == 1:
        assert info == expect[1:2], (what, info, expect)
    else:
        assert info == expect, (what, info, expect)


def same_arrays(a, b, what):
    for x, y in zip(a, b):
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), (what, f)


def address_keys(c, tables):
    """(n, 44) keys: every address the given tables store (300 of a large table's), every
    record's address, the base case's neigh_cases queries, 32 absent addresses."""
    rng = np.random.default_rng([0x5E6] + list(c.name.encode()))
    fams, addrs = [], []
    for t in tables:
        if not len(t):
            continue
        fam, st = nc.family(t), nc.stored(t)
        if len(st) > 300:
            st = [st[int(j)] for j in rng.permutation(len(st))[:300]]
        fams += [fam] * len(st)
        addrs += st
    for fam in ("arp", "ndp"):
        fams += [fam] * 16
        addrs += [nc._random_key(fam, rng) for _ in range(16)]
    recs, _ = gpu.ctrl_writes_host(c.wl.frames, c.wl.desc)
    parts = [rc.key_bytes(fams, addrs, rng), pc.record_keys(recs, rng)]
    if c.base:
        parts.append(rc.queries(c.base)[0])
    return np.concatenate(parts)


def snapshot_equals_arrays(w, kb, arp, ndp, what):
    """The loaded snapshot, a snapshot compiled from the host arrays, and the reference's probe
    over the arrays answer every key alike."""
    image = gpu.NeighImage(arp, ndp)
    try:
        loaded, compiled = gpu_resolve(w, kb), gpu_resolve(w, kb, image=image)
    finally:
        image.free()
    host = neigh.resolve_keys(arp, ndp, rc.as_keys(kb))
    bad = np.nonzero((loaded != compiled) | (loaded != host))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {len(kb)} keys, first {int(bad[0])}: loaded "
                           f"{int(loaded[bad[0]]):#x} compiled {int(compiled[bad[0]]):#x} host "
                           f"{int(host[bad[0]]):#x}")
    return loaded


def both_calls(factory, c, r, what, stream=None):
    """Both calls on fresh contexts and copies of the tables: each against the oracle, the two
    against each other.  Returns the resident call's open worker, outputs and arrays."""
    with factory(c.wl.capacity) as w:
        w.configure(c.wl)
        arp_o, ndp_o = c.wl.arp.copy(), c.wl.ndp.copy()
        old, info = call(w, "segmented", c.wl, arp_o, ndp_o, stream)
    check(old, info, arp_o, ndp_o, c, r, what + " segmented")
    w = factory(c.wl.capacity)
    try:
        w.configure(c.wl)
        arp, ndp = c.wl.arp.copy(), c.wl.ndp.copy()
        new, info = call(w, "resident", c.wl, arp, ndp, stream)
        check(new, info, arp, ndp, c, r, what + " resident")
        for x, y, f in zip(old, new, ("frames", "verdict", "counters", "rule_stats", "l1")):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), f"{what}: {f}"
        same_arrays((arp_o, ndp_o), (arp, ndp), what)
        applied = (arp["update_at"] == NOW).sum() + (ndp["update_at"] == NOW).sum()
        assert bool(applied) == bool(c.expect[1]), what
    except BaseException:
        w.close()
        raise
    return w, arp, ndp


@pytest.mark.parametrize("name", sc.ALL)
def test_case(gpu_worker_factory, monkeypatch, name):
    """Every case through both calls on fresh contexts, then the resident call a second time on
    the same context with the same batch uploaded again: every record is then a refresh
    (rebuilds == 0), and after each call the loaded snapshot equals the returned arrays.

    Branches of upe_segment.hip by case — place:first / last: a cut at packet 0, no trailing
    segment; adjacent2 / adjacent3 / only8: segments of one packet, a batch of nothing else;
    port: the record taken before the in-place reply; norecord:*: ci.ctrl > ci.writes, the second
    listing pass (upe_ctrl_mark plus upe_gpu_compact) and `rec[j].index != k`, norecord:all with
    j == rec.size() from the start; notable:* and norecord:arp: the `continue` at capacity 0 and
    `if (arp_capacity)` / `if (ndp_capacity)` of the older call; count:64 / 65: the first call's
    64 records of room and the retry with writes + writes / 4; count:1023 / 1024 / 1025: the
    kEager boundary and the second copy; count:1025:alt: patches and rebuilds interleaved behind
    it; tables:*: upe_neigh_lookup_host on the host arrays against the patch of the snapshot —
    hidden entries, an address in two slots, stale addresses, wrapped chains, the zero address.
    (count:1025 and count:1025:alt take about 0.2 s each on an MI355X.)"""
    _set_mode(monkeypatch, "default")
    c, r = sc.case(name), sc.oracle_of(name)
    w, arp, ndp = both_calls(gpu_worker_factory, c, r, name)
    try:
        kb = address_keys(c, (c.wl.arp, c.wl.ndp, arp, ndp))
        snapshot_equals_arrays(w, kb, arp, ndp, name)
        r2 = sc.oracle_run(c, start=r)
        got, info = call(w, "resident", c.wl, arp, ndp)
        check(got, info, arp, ndp, c, r2, name + " again",
              (c.expect[0], c.expect[1], c.expect[1], 0))
        snapshot_equals_arrays(w, kb, arp, ndp, name + " again")
    finally:
        w.close()


@pytest.mark.parametrize("n", [64, 65])
def test_first_call_sizing(gpu_worker_factory, n):
    """A fresh context has room for 64 records: count:64 fits, count:65 (`ci.writes > cap`) runs
    upe_gpu_ctrl_writes again with room for 81.  Seen through the outputs alone: all n records
    are applied in order, the last probe leaves with the MAC that names rank n - 1."""
    c, r = sc.case(f"count:{n}"), sc.oracle_of(f"count:{n}")
    with gpu_worker_factory(c.wl.capacity) as w:
        w.configure(c.wl)
        arp, ndp = c.wl.arp.copy(), c.wl.ndp.copy()
        got, info = call(w, "resident", c.wl, arp, ndp)
    check(got, info, arp, ndp, c, r, c.name)
    assert info == (n, n, n, 0)
    i, _, m = c.probes[-1]
    o = int(c.wl.desc[i] >> np.uint64(16))
    assert got[0][o:o + 6].tobytes() == m == sc.mac(0xC0, n - 1)
    slot = nc.Probe(arp).slot(sc.HELD16[(n - 1) % 16])
    assert arp["mac"][slot].tobytes() == m and arp["update_at"][slot] == NOW


def test_scratch_left_behind(gpu_worker_factory):
    """One context: count:1025 (the record scratch grows to room for 1281 records), then
    place:first:new (one record, `cap` derived from the scratch a previous call left, above
    kEager: the eager copy stops at 1024 records), then count:65, then a batch without control
    packets (`ci.writes == 0`, one classify); each against the oracle continued from the call
    before, under its own tables.  Afterwards a plain upe_gpu_process of config-B-small equals the
    reference's golden outputs."""
    plain = sc.without(sc.case("place:first:held"), 0)
    plain = sc.SegCase("no control", plain.wl, (0, 0, 0, 0), (), (), (), plain.wl.n)
    wlb, refb = golden_io.load("config_b_small")
    assert wlb.capacity == plain.wl.capacity
    r = None
    with gpu_worker_factory(wlb.capacity) as w:
        for c in (sc.case("count:1025"), sc.case("place:first:new"), sc.case("count:65"), plain):
            if r is None:
                w.configure(c.wl)
            else:   # the same rules and port; counters, rule_stats and L1 carry over
                w.load_neigh(c.wl.arp, c.wl.ndp)
                r = oracle.Result(None, None, r.counters, r.rule_stats, r.l1, c.wl.arp, c.wl.ndp)
            r = sc.oracle_run(c, start=r)
            arp, ndp = c.wl.arp.copy(), c.wl.ndp.copy()
            got, info = call(w, "resident", c.wl, arp, ndp)
            check(got, info, arp, ndp, c, r, c.name)
            kb = address_keys(c, (c.wl.arp, c.wl.ndp, arp, ndp))
            snapshot_equals_arrays(w, kb, arp, ndp, c.name)
        w.reset_stats()
        w.configure(wlb)
        _assert_same(gpu.run_workload(wlb, worker=w), refb, "config B small afterwards")


STREAMED = ([f"place:{p}:{f}" for p in sc.PLACES for f in sc.FORMS] +
            [f"norecord:{x}" for x in ("ns", "na", "arp", "all")] + ["count:65"])


@pytest.mark.parametrize("name", STREAMED)
def test_callers_stream(gpu_worker_factory, name):
    """Both calls on a stream of the caller's: the batch uploaded on that stream with nothing
    waited for, the outputs fetched on the context's stream after the call returns (the calls
    are synchronous at return).  The rebuild path drains the caller's stream before
    upe_gpu_load_neigh (`s != c->stream`); the patch path queues upe_gpu_neigh_patch on it
    between two classify launches with no synchronisation."""
    hip = _hip()
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    try:
        c, r = sc.case(name), sc.oracle_of(name)
        w, arp, ndp = both_calls(gpu_worker_factory, c, r, name + " on a caller's stream",
                                 stream=s.value)
        try:
            kb = address_keys(c, (c.wl.arp, c.wl.ndp, arp, ndp))
            snapshot_equals_arrays(w, kb, arp, ndp, name)
        finally:
            w.close()
    finally:
        assert hip.hipStreamDestroy(s) == 0


MATCHED = ["tables:wrap", "tables:embed:wrap"] + [f"place:adjacent3:{f}:{s}"
                                                  for f in sc.FORMS for s in ("staged", "memory")]


@pytest.mark.parametrize("mode", ["scan", "tree", "tss"])
@pytest.mark.parametrize("name", MATCHED)
def test_matchers(gpu_worker_factory, monkeypatch, name, mode):
    """200 rules under each forced matcher (the neighbour indexes sit elsewhere in the LDS
    carve-up), the neighbour indexes staged in LDS (16-slot tables; 4096-slot tables of at most
    1638 reachable entries, which the batch's new addresses do not take past it) and read from
    memory (embedded in 8192 slots; 1639 reachable entries and more)."""
    _set_mode(monkeypatch, mode)
    c, r = sc.case(name, 200), sc.oracle_of(name, 200)
    w, arp, ndp = both_calls(gpu_worker_factory, c, r, f"{name} {mode}")
    try:
        assert w.rule_index_kind() == {"scan": 0, "tss": 1, "tree": 2}[mode]
        kb = address_keys(c, (c.wl.arp, c.wl.ndp, arp, ndp))
        snapshot_equals_arrays(w, kb, arp, ndp, f"{name} {mode}")
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------

def _raw(which, ctx, f, d, v, n, arp, acap, ndp, ncap, out):
    fn = getattr(gpu.LIB, "upe_gpu_process_" + ("segmented" if which == "segmented"
                                                else "segmented_resident"))
    rc_ = fn(ctx, f, d, v, n, arp, acap, ndp, ncap, NOW, out, None)
    return rc_, gpu.LIB.upe_gpu_last_error().decode()


@pytest.mark.parametrize("which", CALLS)
def test_refused_calls_change_nothing(gpu_worker_factory, which):
    """The argument checks of both calls, all with n > 0: a NULL context, NULL frames, desc and
    verdict, a NULL table with a nonzero capacity, capacities 3 and 6, n = 2^32.  Each returns -1
    with a message before anything is launched, and the host arrays, counters, rule_stats, L1 and
    the loaded snapshot are byte for byte what they were.  (include/upe_gpu.h says nothing about
    *n_writes / *info after a refused call, so nothing is asserted of them.)"""
    c = sc.case("place:adjacent3:held")
    r = sc.oracle_of(c.name)
    with gpu_worker_factory(c.wl.capacity) as w:
        w.configure(c.wl)
        arp, ndp = c.wl.arp.copy(), c.wl.ndp.copy()
        got, info = call(w, which, c.wl, arp, ndp)
        check(got, info, arp, ndp, c, r, c.name)
        kb = address_keys(c, (c.wl.arp, c.wl.ndp, arp, ndp))

        def state():
            cn, st = w.get_stats()
            return (arp.tobytes(), ndp.tobytes(), cn.tobytes(), st.tobytes(), w.get_l1().tobytes(),
                    gpu_resolve(w, kb).tobytes())

        before = state()
        b = Dev(w, c.wl)
        out = np.zeros(4, np.uint64)
        po = out.ctypes.data
        f, d, v, n = b.frames, b.desc, b.verdict, b.n
        pa, pn, ca, cn_ = arp.ctypes.data, ndp.ctypes.data, len(arp), len(ndp)
        ctx = w._ctx
        refused = [("context", (None, f, d, v, n, pa, ca, pn, cn_)),
                   ("batch buffer", (ctx, None, d, v, n, pa, ca, pn, cn_)),
                   ("batch buffer", (ctx, f, None, v, n, pa, ca, pn, cn_)),
                   ("batch buffer", (ctx, f, d, None, n, pa, ca, pn, cn_)),
                   ("neighbour table", (ctx, f, d, v, n, None, ca, pn, cn_)),
                   ("neighbour table", (ctx, f, d, v, n, pa, ca, None, cn_)),
                   ("powers of two", (ctx, f, d, v, n, pa, 3, pn, cn_)),
                   ("powers of two", (ctx, f, d, v, n, pa, ca, pn, 6)),
                   ("too large", (ctx, f, d, v, 1 << 32, pa, ca, pn, cn_))]
        for word, args in refused:
            rc_, msg = _raw(which, *args, po)
            assert rc_ == -1 and word in msg, (word, rc_, msg)
            assert state() == before, word
        frames, verdict = b.fetch()
        assert np.array_equal(frames, c.wl.frames), "a refused call wrote into the batch"
        # and the context goes on: the same batch again, every record a refresh
        r2 = sc.oracle_run(c, start=r)
        got, info = call(w, which, c.wl, arp, ndp)
        expect = (c.expect[0], c.expect[1], c.expect[1], 0)
        check(got, info, arp, ndp, c, r2, c.name + " after refused calls", expect)


def _unplaceable():
    """Three NDP addresses of one fold_v6 held (tests/neigh_cases.py one_fold: they share all
    three candidate slots of the index), the fourth taught by an NA in the middle of the batch:
    upe_gpu_load_neigh cannot place it.  Returns (case, the four addresses)."""
    four = nc.one_fold_keys(4)
    b = sc._Batch()
    m = sc.mac(0x41, 0)
    for k in four[:3]:
        b.probe(k, "old")
    b.ctrl(sc.teach(four[3], m, 1), "rebuild")
    b.probe(four[3], "new", m)
    for k in four[:3]:
        b.probe(k, "old")
    arp = sc.tables((sc.Y4,))[0]
    return b.done("unplaceable", arp, nc.table("ndp", "one_fold").copy()), four


@pytest.mark.parametrize("which", CALLS)
def test_failed_load_mid_batch(gpu_worker_factory, which):
    """A table write whose upe_gpu_load_neigh fails: the call returns -1 with that call's
    message; the snapshot loaded before the write stays loaded and still answers (the three held
    addresses, not the fourth); the context then runs a following batch correctly from the state
    it reports.  include/upe_gpu.h promises nothing more about the partly processed batch, and
    nothing more is asserted."""
    c, four = _unplaceable()
    recs, info = gpu.ctrl_writes_host(c.wl.frames, c.wl.desc)
    assert len(recs) == 1 and recs["kind"][0] == CW_NDP and recs["ip"][0].tobytes() == four[3]
    follow = sc.without(c, c.cuts[0])
    with gpu_worker_factory(c.wl.capacity) as w:
        w.configure(c.wl)
        kb = rc.key_bytes(["ndp"] * 4 + ["arp"], four + [sc.Y4], np.random.default_rng(4))
        want = neigh.resolve_keys(c.wl.arp, c.wl.ndp, rc.as_keys(kb))
        assert (want[:3] != 0).all() and want[3] == 0 and want[4] != 0
        assert np.array_equal(gpu_resolve(w, kb), want)
        arp, ndp = c.wl.arp.copy(), c.wl.ndp.copy()
        b = Dev(w, c.wl)
        out = np.zeros(4, np.uint64)
        rc_, msg = _raw(which, w._ctx, b.frames, b.desc, b.verdict, b.n, arp.ctypes.data, len(arp),
                        ndp.ctypes.data, len(ndp), out.ctypes.data)
        b.fetch()
        assert rc_ == -1 and "placement" in msg, (rc_, msg)
        assert np.array_equal(gpu_resolve(w, kb), want), "the snapshot before the write"
        # a following batch, from the counters, rule_stats and L1 the context reports
        cn, st = w.get_stats()
        start = oracle.Result(None, None, cn, st, w.get_l1(), c.wl.arp, c.wl.ndp)
        r = sc.oracle_run(follow, start=start)
        a2, n2 = c.wl.arp.copy(), c.wl.ndp.copy()
        got, info = call(w, which, follow.wl, a2, n2)
        _assert_same(got, _ref(r), "the batch after the failed load")
        assert info == ((0,) if which == "segmented" else (0, 0, 0, 0))
