"""rule_stats and counters of the GPU path at every width and boundary the accounting assumes.

The tables and batches of tests/accounting_cases.py (pinned on the CPU by
tests/test_accounting_cases.py) through the kernels: get_stats() must equal the generator's
bincount bit for bit, and every verdict's code and rule bits its target.  Table sizes sit on the
switches between the three accounting routes (replicated accumulators, per-index replicas, the
group-by) and on the group-by's range and key limits; batch sizes on either side of its vector /
tail split and of a chunk; batches aim every packet at one boundary index, hit every rule a
different number of times with its own length, match nothing, or mix both inside every 64-packet
group.  The same totals must come out of every launch form, add up over launches, vanish on
reset_stats, follow rule_ids over a table change, survive the flush that skips the counting wave
(look-back live) and each forced matcher, and hold when one rule takes more bytes than eight
workgroups' 32-bit bins could (UPE_GPU_GRID_CAP=8).
"""
from __future__ import annotations

import time

import numpy as np
import pytest

import accounting_cases as ac
from test_accounting_cases import CODE_AND_RULE, MOST
from test_gpu_rule_tables import _set_mode
from upe_amd import gpu, synth

pytestmark = pytest.mark.gpu

FORM_TABLES = (ac.SMALL_LAST, 1000, ac.LDS_LAST + 1)   # small, mid-size, group-by


def _open(factory, t, capacity=None):
    w = factory(t.capacity if capacity is None else capacity)
    w.load_rules(t.rules_sorted)
    arp, ndp = ac.neighbours()
    w.load_neigh(arp, ndp)
    w.set_port(synth.PORT_MAC, synth.PORT_IP4)
    w.set_l1(synth.l1_zero())
    return w


def _assert_totals(w, t, batches, what, tables=None):
    """get_stats() equals the bincount of `batches` (each over table `tables[k]`, default t)."""
    c, s = w.get_stats()
    want_c = np.zeros_like(c)
    want_s = np.zeros_like(s)
    for k, b in enumerate(batches):
        tc, ts = ac.expected(tables[k] if tables else t, [b], capacity=w.capacity)
        for f in want_c.dtype.names:
            want_c[f] += tc[f]
        want_s["packets"] += ts["packets"]
        want_s["bytes"] += ts["bytes"]
    bad = np.nonzero((s["packets"] != want_s["packets"]) | (s["bytes"] != want_s["bytes"]))[0]
    assert bad.size == 0, (f"{what}: rule_stats differ at {bad.size} rule ids, first "
                           f"{[(int(r), s[r].tolist(), want_s[r].tolist()) for r in bad[:4]]}")
    assert c.tobytes() == want_c.tobytes(), f"{what}: counters {c} != {want_c}"


def _assert_verdict(t, b, verdict, what):
    bad = np.nonzero((verdict & CODE_AND_RULE) != ac.expected_verdict(t, b))[0]
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first {bad[:4].tolist()}"


def _single(w, t, b, emit, what):
    d = gpu.DeviceBatch(w, b.frames, b.desc)
    (d.run_emit if emit else d.run)()
    _, verdict = d.fetch()
    d.free()
    _assert_verdict(t, b, verdict, what)


# ---------------------------------------------------------------------------------------------
# every table x every batch shape
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrules", ac.TABLE_SIZES)
def test_table_by_shape(gpu_worker_factory, monkeypatch, nrules):
    _set_mode(monkeypatch, "default")
    t = ac.table(nrules)
    t0 = time.perf_counter()
    w = _open(gpu_worker_factory, t)
    done = []
    try:
        for n in ac.BATCH_SIZES:
            # (past a chunk, "every" and "interleaved" hit the whole table, or where the batch has
            # no room for that a stride through every range: ac.most_for, pinned on the CPU)
            for b in ac.shapes(t, n):
                for emit in (False, True):
                    what = f"{nrules} rules {b.name} emit={emit}"
                    _single(w, t, b, emit, what)
                    done.append(b)
                    # totals after every launch for the batches that cross a chunk or a range,
                    # once per size for the rest (a wrong total is still caught, by its size)
                    if n > ac.K_HIST_CHUNK_MIN or b.name.startswith(("every", "interleaved")):
                        _assert_totals(w, t, done, what)
            _assert_totals(w, t, done, f"{nrules} rules after n={n}")
        info = w.launch_info()
    finally:
        w.close()
    assert info["launches"] >= len(done)
    print(f"{nrules} rules ({t.path}): {len(done)} launches, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------
# every launch form
# ---------------------------------------------------------------------------------------------

FORMS = ("rss", "emit_tx", "batches", "batches_emit", "queue_emit", "ring_emit", "segmented",
         "host", "host_emit", "mapped", "mapped_emit")
N_FORM = 2 * ac.K_HIST_CHUNK_MIN + 1 + 1024   # 17409: three group-by chunks, a ragged last group


@pytest.mark.parametrize("nrules", FORM_TABLES)
@pytest.mark.parametrize("form", FORMS)
def test_launch_forms(gpu_worker_factory, monkeypatch, form, nrules):
    _set_mode(monkeypatch, "default")
    t = ac.table(nrules)
    b = ac.every_rule(t, 16 * 1024 if form == "ring_emit" else N_FORM)
    n, times = b.n, 1
    verdict = None
    w = _open(gpu_worker_factory, t)
    try:
        if form in ("host", "host_emit"):
            frames, verdict = b.frames.copy(), np.zeros(n, np.uint32)
            if form == "host":
                w.process_host(frames, b.desc, verdict, 1000)     # launches of 1000 packets
            else:
                w.process_host_emit(frames, b.desc, verdict, np.zeros((n, 16), np.uint8), 1000, 0)
            assert w.launch_info()["launches"] >= n // 1000
        elif form in ("mapped", "mapped_emit"):
            pins = [gpu.PinnedArray(b.frames.shape, np.uint8), gpu.PinnedArray((n,), np.uint64),
                    gpu.PinnedArray((n,), np.uint32), gpu.PinnedArray((n, 16), np.uint8)]
            try:
                pins[0].array[:] = b.frames
                pins[1].array[:] = b.desc
                if form == "mapped":
                    w.process_mapped(pins[0].array, pins[1].array, pins[2].array)
                else:
                    w.process_mapped_emit(pins[0].array, pins[1].array, pins[2].array, pins[3].array)
                w.sync()
                verdict = pins[2].array.copy()
            finally:
                for p in pins:
                    p.free()
        else:
            d = gpu.DeviceBatch(w, b.frames, b.desc)
            d.hdr = w.malloc(16 * n)
            extra = []
            if form == "rss":
                extra = [w.malloc(4 * n)]
                w.process_rss(d.frames, d.desc, d.verdict, extra[0], n)
            elif form == "emit_tx":
                extra = [w.malloc(4 * n), w.malloc(4 * ((n + 63) // 64))]
                w.process_emit_tx(d.frames, d.desc, d.verdict, d.hdr, extra[0], extra[1], n)
            elif form == "batches":
                times = 3   # the same descriptors three times (a forwarded frame's TTL 64 -> 61)
                w.process_batches([d.frames] * times, d.desc, d.verdict, n)
            elif form == "batches_emit":
                times = 3
                w.process_batches_emit([d.frames] * times, d.desc, d.verdict, d.hdr, n)
            elif form == "queue_emit":
                cuts = [0, 1001, 5003, ac.K_HIST_CHUNK_MIN + 17, n]   # no multiple of 64
                assert all(c % 64 for c in cuts[1:])
                # (records are 16-byte aligned at any packet index)
                w.process_queue_emit([(d.frames, d.desc + 8 * s, d.verdict + 4 * s, d.hdr + 16 * s,
                                       e - s) for s, e in zip(cuts[:-1], cuts[1:])])
            elif form == "ring_emit":
                w.process_ring_emit(d.frames, d.desc, d.verdict, d.hdr, 1024, n // 1024)
            else:
                arp, ndp = ac.neighbours()
                assert w.process_segmented(d.frames, d.desc, d.verdict, n, arp, ndp) == 0
            _, verdict = d.fetch()
            for p in extra:
                w.free(p)
            d.free()
        _assert_totals(w, t, [b] * times, f"{form} {nrules} rules")
    finally:
        w.close()
    _assert_verdict(t, b, verdict, f"{form} {nrules} rules")


# ---------------------------------------------------------------------------------------------
# accumulation, reset, a table of another route
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrules,then", [(ac.SMALL_LAST, 1000), (1000, ac.LDS_LAST + 1),
                                         (ac.LDS_LAST + 1, 8), (ac.K_GB_PACKED + 1, 1000)])
def test_accumulate_reset_reload(gpu_worker_factory, monkeypatch, nrules, then):
    _set_mode(monkeypatch, "default")
    t, t2 = ac.table(nrules), ac.table(then)
    cap = max(t.capacity, t2.capacity)
    b1, b2 = ac.every_rule(t, N_FORM), ac.interleaved(t, ac.K_HIST_CHUNK_MIN + 15)
    b3 = ac.every_rule(t2, N_FORM)
    for b in (b1, b2):   # a table past what the batch has room for is hit by a stride, in every range
        assert all(((b.target >= r0 + 2) & (b.target < r1 - 2)).any() or r1 - r0 < 5
                   for r0, r1 in ac.ranges(t)), b.name
    w = _open(gpu_worker_factory, t, cap)
    try:
        _single(w, t, b1, False, "first")
        _assert_totals(w, t, [b1], f"{nrules}: once")
        _single(w, t, b1, True, "second")
        _assert_totals(w, t, [b1, b1], f"{nrules}: twice")
        w.reset_stats()
        c, s = w.get_stats()
        assert not s["packets"].any() and not s["bytes"].any(), f"{nrules}: rule_stats after reset"
        assert c.tobytes() == np.zeros_like(c).tobytes(), f"{nrules}: counters after reset"
        _single(w, t, b2, False, "after reset")
        _assert_totals(w, t, [b2], f"{nrules}: only the batch after the reset")
        # another table, of another accounting route: what rule ids took so far stays theirs
        w.load_rules(t2.rules_sorted)
        _assert_totals(w, t, [b2], f"{nrules} -> {then}: carried over by rule id")
        _single(w, t2, b3, True, "new table")
        _assert_totals(w, t, [b2, b3], f"{nrules} -> {then}: both tables' hits",
                       tables=[t, t2])
        # the SIGHUP reload: the old array handed back as it stood, a fresh one from zero
        old = w.reload_rules(t.rules_sorted, cap)
        want = np.zeros_like(old)
        for tt, b in ((t, b2), (t2, b3)):
            ts = ac.expected(tt, [b], capacity=cap)[1]
            want["packets"] += ts["packets"]
            want["bytes"] += ts["bytes"]
        assert np.array_equal(old, want), f"{then} -> {nrules}: rule_stats handed back"
        _single(w, t, b1, False, "after the reload")
        c, s = w.get_stats()
        assert np.array_equal(s, ac.expected(t, [b1], capacity=cap)[1]), "fresh rule_stats"
        assert int(c["pkts_in"][0]) == b2.n + b3.n + b1.n   # a reload keeps the counters
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------
# the mid-size flush while the look-back is live
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("emit", [False, True], ids=["inplace", "emit"])
@pytest.mark.parametrize("nrules", [ac.SMALL_LAST + 1, 1000, ac.LDS_LAST])
def test_lookback_live_flush(gpu_worker_factory, monkeypatch, nrules, emit):
    """A starting L1 entry that contradicts the ARP table keeps the look-back kernel, whose
    workgroups flush their bins without the counting wave (another start and stride): every
    sorted index is hit, each with its own count and length."""
    _set_mode(monkeypatch, "default")
    monkeypatch.setenv("UPE_GPU_NOLB", "0")
    t = ac.table(nrules)
    b = ac.every_rule(t, 40005)
    assert len(np.unique(b.target)) == nrules
    l1 = synth.l1_zero()
    l1["last_arp_ip"] = ac.ARP_IP
    l1["last_arp_mac"] = np.frombuffer(bytes.fromhex("0badc0ffee01"), np.uint8)
    w = _open(gpu_worker_factory, t)
    try:
        for k in range(2):   # the second launch starts from the same disagreeing entry
            w.set_l1(l1)
            _single(w, t, b, emit, f"{nrules} rules launch {k}")
            info = w.launch_info()
            assert not info["variant"] & gpu.VAR_NOLB, info
            _assert_totals(w, t, [b] * (k + 1), f"look-back live, {nrules} rules, launch {k}")
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------
# forced matchers
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["scan", "tree"])
@pytest.mark.parametrize("nrules", [1000, ac.K_HIST_RANGE])
def test_forced_matchers(gpu_worker_factory, monkeypatch, nrules, mode):
    _set_mode(monkeypatch, mode)
    t = ac.table(nrules)
    batches = [ac.every_rule(t, 2 * ac.K_HIST_CHUNK_MIN + 1, MOST), ac.interleaved(t, 4097, MOST)]
    batches += [ac.one_rule(t, idx, 65, which) for which, idx in t.boundaries().items()]
    w = _open(gpu_worker_factory, t)
    try:
        for k, b in enumerate(batches):
            _single(w, t, b, bool(k % 2), f"{mode} {nrules} rules {b.name}")
            scan = w.launch_info()["variant"] & gpu.VAR_SCAN
            assert (scan == gpu.VAR_TREE) if mode == "tree" else scan in (gpu.VAR_FAM, gpu.VAR_GLB)
            _assert_totals(w, t, batches[:k + 1], f"{mode} {nrules} rules {b.name}")
        assert w.rule_index_kind() == (2 if mode == "tree" else 0)
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------
# more bytes on one rule than the grid's 32-bit bins hold
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", ["8", None], ids=["grid8", "uncapped"])
@pytest.mark.parametrize("nrules", [8, 1000])
def test_byte_bin(gpu_worker_factory, monkeypatch, nrules, cap):
    """2^20 descriptors of 65535 bytes on one dropping rule: 2^36 bytes.  Eight workgroups with a
    32-bit byte bin each hold 2^35 at most, so on a grid capped at 8 some bin would have to wrap;
    the host cuts the launch so that no workgroup takes more than kWgPackets packets
    (upe_plan.h launch_limit).  Before that limit existed this test failed with the cap set."""
    _set_mode(monkeypatch, "default")
    if cap is None:
        monkeypatch.delenv("UPE_GPU_GRID_CAP", raising=False)
    else:
        monkeypatch.setenv("UPE_GPU_GRID_CAP", cap)
    t = ac.table(nrules)
    b = ac.byte_bin_batch(t)
    w = _open(gpu_worker_factory, t)
    try:
        for k, emit in enumerate((False, True)):
            _single(w, t, b, emit, f"byte bin {nrules} rules emit={emit}")
            grid = w.launch_info()["grid"]
            print(f"byte bin: {nrules} rules, cap {cap}, emit={emit}: grid {grid}")
            if cap is not None:
                assert grid <= 8 and b.n * 65535 > grid << 32
            _assert_totals(w, t, [b] * (k + 1), f"byte bin {nrules} rules cap {cap} emit={emit}")
        rid = int(t.rule_id[b.target[0]])
        s = w.get_stats()[1]
        assert s[rid].tolist() == (2 << 20, (2 << 20) * 65535)
    finally:
        w.close()
