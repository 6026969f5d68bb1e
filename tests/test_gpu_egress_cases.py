"""GPU: emit records, the in-pass egress list and upe_gpu_compact on chosen forwarded sets.

The batches of tests/egress_cases.py (pinned on the CPU by tests/test_egress_cases.py) through
every emit launch form.  Every output buffer is filled with a poison no record, index or count
can equal before the call and has 64 more records, or entries, behind it; the whole raw array is
compared with the one laid out from the restatement's answers, bit for bit: a record in the wrong
slot, a write to a slot the layout leaves alone ("the other slots are not written", "slots past a
group's count are not written": include/upe_gpu.h), a missing count of a group that forwards
nothing, and anything past the end all differ from it.
"""
from __future__ import annotations

import time

import numpy as np
import pytest

import accounting_cases as ac
import egress_cases as ec
from test_egress_cases import exp_of
from test_gpu_gate_matrix import _default_mode, _set_mode
from upe_amd import gpu, synth
from upe_amd.layout import V_FWD

pytestmark = pytest.mark.gpu

VAR_EMIT, VAR_TSS, VAR_LEAN = 1, 2, 4


class Dev:
    """Device arrays filled from host ones, read back whole."""

    def __init__(self, w):
        self.w = w
        self.ptrs = []

    def put(self, host: np.ndarray) -> int:
        host = np.ascontiguousarray(host)
        p = self.w.malloc(max(host.nbytes, 16))
        self.ptrs.append(p)
        if host.nbytes:
            self.w.h2d(p, host)
            self.w.sync()
        return p

    def poison(self, nbytes: int) -> int:
        return self.put(np.full(nbytes, ec.POISON, np.uint8))

    def get(self, p: int, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype)
        self.w.sync()
        if out.nbytes:
            self.w.d2h(out, p)
            self.w.sync()
        return out

    def free(self) -> None:
        for p in self.ptrs:
            self.w.free(p)
        self.ptrs = []


def _open(factory, t, big, l1=None):
    w = factory(t.capacity)
    w.load_rules(t.rules_sorted)
    w.load_neigh(*ec.neighbours(big))
    w.set_port(synth.PORT_MAC, synth.PORT_IP4)
    w.set_l1(synth.l1_zero() if l1 is None else l1)
    return w


def _mode(monkeypatch, mode):
    _default_mode(monkeypatch) if mode == "default" else _set_mode(monkeypatch, mode)


def _assert_verdict(got, want, what):
    n = len(want)
    bad = np.nonzero(got[:n] != want)[0]
    assert bad.size == 0, (f"{what}: {bad.size} verdicts differ, first packet {int(bad[0])} (group "
                           f"{int(bad[0]) // 64}): want {int(want[bad[0]]):#x}, got "
                           f"{int(got[bad[0]]):#x}")
    assert (got[n:] == ec.POISON32).all(), f"{what}: a verdict written past the batch"


def _assert_state(w, e, what):
    c, s = w.get_stats()
    assert c.tobytes() == e.counters.tobytes(), f"{what}: counters {c} != {e.counters}"
    assert np.array_equal(s, e.rule_stats), f"{what}: rule_stats"
    assert w.get_l1().tobytes() == e.l1.tobytes(), f"{what}: L1 state"


def _assert_frames(got, e, what):
    bad = np.nonzero(got != e.frames)[0]
    assert bad.size == 0, f"{what}: {bad.size} frame bytes differ, first at offset {int(bad[0])}"


def _launch(w, b, e, with_tx, what, l1=None):
    """One batch through upe_gpu_process_emit or _emit_tx from fresh counters and the given L1
    state; every output against e.  Returns launch_info()."""
    n = b.n
    d = Dev(w)
    try:
        frames, desc = d.put(b.frames), d.put(b.desc)
        verdict = d.poison(4 * (n + ec.CANARY))
        hdr = d.poison(16 * (n + ec.CANARY))
        tx = d.poison(4 * (n + ec.CANARY))
        cnt = d.poison(4 * (e.groups + ec.CANARY))
        w.set_l1(synth.l1_zero() if l1 is None else l1)
        w.reset_stats()
        if with_tx:
            w.process_emit_tx(frames, desc, verdict, hdr, tx, cnt, n)
        else:
            w.process_emit(frames, desc, verdict, hdr, n)
        info = w.launch_info()
        _assert_verdict(d.get(verdict, n + ec.CANARY, np.uint32), e.verdict, what)
        ec.check_expected(e, what, raw=d.get(hdr, (n + ec.CANARY, 16), np.uint8))
        got_tx = d.get(tx, n + ec.CANARY, np.uint32)
        got_cnt = d.get(cnt, e.groups + ec.CANARY, np.uint32)
        if with_tx:
            ec.check_expected(e, what, tx=got_tx, tx_count=got_cnt)
        else:
            assert (got_tx == ec.POISON32).all() and (got_cnt == ec.POISON32).all()
        _assert_frames(d.get(frames, b.frames.shape, np.uint8), e, what)
        _assert_state(w, e, what)
    finally:
        d.free()
    assert info["variant"] & VAR_EMIT, what
    assert (info["variant"] & gpu.VAR_TX == gpu.VAR_TX) == with_tx, (what, info)
    if not with_tx:
        assert not info["variant"] & gpu.VAR_TX, (what, info)   # the plain device path
    return info


# ---------------------------------------------------------------------------------------------
# a. every kernel family, upe_gpu_process_emit and upe_gpu_process_emit_tx
# ---------------------------------------------------------------------------------------------

FAMILIES = [("default", 8), ("default", 1000), ("default", ac.LDS_LAST + 1), ("scan", 1000),
            ("tree", 1000), ("tree-memory", 1000), ("tss", 1000), ("tss-unstaged", 1000),
            # (the largest table is matched through the tuple space by default: forced to a scan
            # and to the tree, the launch writes the group-by's side array and is never lean)
            ("scan", ac.LDS_LAST + 1), ("tree", ac.LDS_LAST + 1)]


def _assert_variant(info, mode, nrules, big, what):
    var = info["variant"]
    tss = bool(var & VAR_TSS)
    scan = var & gpu.VAR_SCAN
    if mode != "default":
        assert tss == mode.startswith("tss"), (what, info)
    if mode.startswith("tree"):
        assert scan == gpu.VAR_TREE, (what, info)
    elif mode == "scan":
        assert scan in (gpu.VAR_FAM, gpu.VAR_GLB), (what, info)
    elif tss or nrules == 8:
        assert scan == 0, (what, info)
    # lean: both neighbour indexes staged in LDS, and no group-by side array (a table past the LDS
    # bins has one unless it is matched through the tuple space: upe_plan.h plan_lds)
    side_array = ac.stats_path(nrules) == "group-by" and not tss
    assert bool(var & VAR_LEAN) == (not big and not side_array), (what, info)


@pytest.mark.parametrize("big", [False, True], ids=["lds", "memory"])
@pytest.mark.parametrize("mode,nrules", FAMILIES, ids=[f"{m}-{n}" for m, n in FAMILIES])
def test_every_kernel_family(gpu_worker_factory, monkeypatch, mode, nrules, big):
    _mode(monkeypatch, mode)
    t = ec.table(nrules)
    t0 = time.perf_counter()
    variants = set()
    w = _open(gpu_worker_factory, t, big)
    try:
        if mode != "default":
            assert w.rule_index_kind() == (1 if mode.startswith("tss") else
                                           2 if mode.startswith("tree") else 0)
        for name, b in ec.sequences().items():
            e = exp_of(name, nrules, big)
            for with_tx in (False, True):
                what = f"{mode} {nrules} rules {'memory' if big else 'lds'} {name} tx={with_tx}"
                info = _launch(w, b, e, with_tx, what)
                _assert_variant(info, mode, nrules, big, what)
                variants.add(info["variant"])
    finally:
        w.close()
    print(f"{mode} {nrules} rules big={big}: variants {sorted(hex(v) for v in variants)}, "
          f"{time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------------------------
# b. whole tiles, several tiles per workgroup
# ---------------------------------------------------------------------------------------------

N_TILED = 3 * 8 * 1024


@pytest.mark.parametrize("big", [False, True], ids=["lds", "memory"])
@pytest.mark.parametrize("nrules", [8, 1000])
def test_several_tiles_per_workgroup(gpu_worker_factory, monkeypatch, nrules, big):
    """Full-width tiles, three to a workgroup of a grid capped at eight: the next chunk's
    prefetch and the persistent loop."""
    _mode(monkeypatch, "default")
    monkeypatch.setenv("UPE_GPU_GRID_CAP", "8")
    t = ec.table(nrules)
    b = ec.tiled(N_TILED)
    e = ec.expected(ec.workload(b, t, big))
    w = _open(gpu_worker_factory, t, big)
    try:
        for with_tx in (False, True):
            info = _launch(w, b, e, with_tx, f"tiled {nrules} rules big={big} tx={with_tx}")
            assert info["grid"] == 8, info
            assert bool(info["variant"] & VAR_LEAN) == (not big), info
    finally:
        w.close()


# ---------------------------------------------------------------------------------------------
# c. every other emit launch form
# ---------------------------------------------------------------------------------------------

FORM_TABLES = (8, ac.LDS_LAST + 1)


def _assert_chain_state(w, chain, what):
    _assert_state(w, chain[-1], what)


@pytest.mark.parametrize("nrules", FORM_TABLES)
def test_batches_emit(gpu_worker_factory, monkeypatch, nrules):
    """Three passes over one d_hdr: the last pass's records at the last pass's slots; a slot only
    an earlier pass forwarded into keeps that pass's record (no pass clears the array)."""
    _mode(monkeypatch, "default")
    t = ec.table(nrules)
    passes = ec.three_passes()
    n = passes[0].n
    chain, state = [], {}
    raw = np.full((n + ec.CANARY, 16), ec.POISON, np.uint8)
    for b in passes:
        e = ec.expected(ec.workload(b, t), **state)
        state = {"l1": e.l1, "counters": e.counters, "rule_stats": e.rule_stats}
        fwd = (e.verdict & 0xF) == V_FWD
        raw[e.slots[fwd]] = e.records[fwd]
        chain.append(e)
    assert not np.array_equal(raw, chain[-1].raw)
    w = _open(gpu_worker_factory, t, False)
    d = Dev(w)
    try:
        frames = [d.put(b.frames) for b in passes]
        desc = d.put(passes[0].desc)
        verdict, hdr = d.poison(4 * (n + ec.CANARY)), d.poison(16 * (n + ec.CANARY))
        w.process_batches_emit(frames, desc, verdict, hdr, n)
        what = f"batches_emit {nrules} rules"
        _assert_verdict(d.get(verdict, n + ec.CANARY, np.uint32), chain[-1].verdict, what)
        ec.check_layout(raw, d.get(hdr, (n + ec.CANARY, 16), np.uint8), what=what)
        for k, b in enumerate(passes):
            _assert_frames(d.get(frames[k], b.frames.shape, np.uint8), chain[k], f"{what} pass {k}")
        _assert_chain_state(w, chain, what)
    finally:
        d.free()
        w.close()


@pytest.mark.parametrize("nrules", FORM_TABLES)
def test_queue_emit(gpu_worker_factory, monkeypatch, nrules):
    """Cuts that are no multiples of 64: each batch's slots are counted from its own hdr pointer."""
    _mode(monkeypatch, "default")
    t = ec.table(nrules)
    b = ec.sequences()["pairs"]
    n = b.n
    cuts = [0, 1001, 1002, 3003, 5555, n]
    assert all(c % 64 for c in cuts[1:-1])
    wl = ec.workload(b, t)
    chain = ec.expected_chain(wl, cuts)
    raw = np.full((n + ec.CANARY, 16), ec.POISON, np.uint8)
    for s, e in zip(cuts, chain):
        fwd = (e.verdict & 0xF) == V_FWD
        raw[s + e.slots[fwd]] = e.records[fwd]
    w = _open(gpu_worker_factory, t, False)
    d = Dev(w)
    try:
        frames, desc = d.put(b.frames), d.put(b.desc)
        verdict, hdr = d.poison(4 * (n + ec.CANARY)), d.poison(16 * (n + ec.CANARY))
        w.process_queue_emit([(frames, desc + 8 * s, verdict + 4 * s, hdr + 16 * s, e - s)
                              for s, e in zip(cuts[:-1], cuts[1:])])
        what = f"queue_emit {nrules} rules"
        _assert_verdict(d.get(verdict, n + ec.CANARY, np.uint32),
                        np.concatenate([e.verdict for e in chain]), what)
        ec.check_layout(raw, d.get(hdr, (n + ec.CANARY, 16), np.uint8), what=what)
        _assert_frames(d.get(frames, b.frames.shape, np.uint8), exp_of("pairs", nrules), what)
        _assert_chain_state(w, chain, what)
    finally:
        d.free()
        w.close()


@pytest.mark.parametrize("nrules", FORM_TABLES)
def test_ring_emit(gpu_worker_factory, monkeypatch, nrules):
    """Eight batches of 1024 packets in one launch, each a different rotation of the pair
    sequence; records are counted from the ring's first packet."""
    _mode(monkeypatch, "default")
    t = ec.table(nrules)
    per, count = 1024, 8
    pair = ec.kinds_of(ec.pair_mask())
    kinds = np.concatenate([np.roll(pair, -977 * j)[:per] for j in range(count)])
    assert len({kinds[j * per:(j + 1) * per].tobytes() for j in range(count)}) == count
    b = ec.build(kinds, "ring")
    n = b.n
    e = ec.expected(ec.workload(b, t))
    w = _open(gpu_worker_factory, t, False)
    d = Dev(w)
    try:
        frames, desc = d.put(b.frames), d.put(b.desc)
        verdict, hdr = d.poison(4 * (n + ec.CANARY)), d.poison(16 * (n + ec.CANARY))
        w.process_ring_emit(frames, desc, verdict, hdr, per, count)
        what = f"ring_emit {nrules} rules"
        _assert_verdict(d.get(verdict, n + ec.CANARY, np.uint32), e.verdict, what)
        ec.check_expected(e, what, raw=d.get(hdr, (n + ec.CANARY, 16), np.uint8))
        _assert_frames(d.get(frames, b.frames.shape, np.uint8), e, what)
        _assert_state(w, e, what)
    finally:
        d.free()
        w.close()


@pytest.mark.parametrize("nrules", FORM_TABLES)
def test_mapped_emit(gpu_worker_factory, monkeypatch, nrules):
    _mode(monkeypatch, "default")
    t = ec.table(nrules)
    b = ec.sequences()["pairs"]
    n = b.n
    e = exp_of("pairs", nrules)
    w = _open(gpu_worker_factory, t, False)
    pins = [gpu.PinnedArray(b.frames.shape, np.uint8), gpu.PinnedArray((n,), np.uint64),
            gpu.PinnedArray((n + ec.CANARY,), np.uint32),
            gpu.PinnedArray((n + ec.CANARY, 16), np.uint8)]
    try:
        pins[0].array[:] = b.frames
        pins[1].array[:] = b.desc
        pins[2].array[:] = ec.POISON32
        pins[3].array[:] = ec.POISON
        w.process_mapped_emit(pins[0].array, pins[1].array, pins[2].array[:n], pins[3].array[:n])
        w.sync()
        what = f"mapped_emit {nrules} rules"
        assert w.launch_info()["variant"] & gpu.VAR_TX == gpu.VAR_HOST, what
        _assert_verdict(pins[2].array.copy(), e.verdict, what)
        ec.check_expected(e, what, raw=pins[3].array.copy())
        _assert_frames(pins[0].array.copy(), e, what)
        _assert_state(w, e, what)
    finally:
        for p in pins:
            p.free()
        w.close()


@pytest.mark.parametrize("chunk", [1000, 0])
@pytest.mark.parametrize("nrules", FORM_TABLES)
def test_host_emit(gpu_worker_factory, monkeypatch, nrules, chunk):
    """Records are counted from the batch's first packet, in whole 64-packet groups: a chunk of
    1000 runs as launches of 960.  h_hdr comes back chunk by chunk in one copy each, so the slots
    that hold no record are overwritten with unspecified bytes (include/upe_gpu.h says so): the
    record slots, and the canary behind the batch, are compared.  apply_threads = -1 leaves the
    frames as emit mode does; 0 gives the frames of the in-place path."""
    _mode(monkeypatch, "default")
    t = ec.table(nrules)
    b = ec.sequences()["pairs"]
    n = b.n
    step = chunk // 64 * 64 if chunk else n
    cuts = list(range(0, n, step)) + [n]
    wl = ec.workload(b, t)
    chain = ec.expected_chain(wl, cuts)
    want_v = np.concatenate([e.verdict for e in chain])
    raw = np.full((n + ec.CANARY, 16), ec.POISON, np.uint8)
    for s, e in zip(cuts, chain):
        fwd = (e.verdict & 0xF) == V_FWD
        raw[s + e.slots[fwd]] = e.records[fwd]
    only = raw[:, 15] != ec.POISON
    only[n:] = True
    one = exp_of("pairs", nrules)
    assert np.array_equal(raw[only], one.raw[only])   # the cuts fall on whole groups
    for threads, want_frames in ((-1, one.frames), (0, one.frames_applied)):
        what = f"host_emit {nrules} rules chunk {chunk} apply_threads {threads}"
        w = _open(gpu_worker_factory, t, False)
        try:
            frames = b.frames.copy()
            verdict = np.full(n + ec.CANARY, ec.POISON32, np.uint32)
            hdr = np.full((n + ec.CANARY, 16), ec.POISON, np.uint8)
            # (the arrays carry their canary: the call is told n records through desc)
            gpu._check(gpu.LIB.upe_gpu_process_host_emit(
                w._ctx, gpu._np_ptr(frames), frames.nbytes, gpu._np_ptr(b.desc),
                gpu._np_ptr(verdict), gpu._np_ptr(hdr), n, chunk, threads), what)
            assert w.launch_info()["launches"] == len(cuts) - 1, what
            _assert_verdict(verdict, want_v, what)
            ec.check_layout(raw, hdr, what=what, only=only)
            bad = np.nonzero(frames != want_frames)[0]
            assert bad.size == 0, f"{what}: frames differ, first at offset {int(bad[0])}"
            _assert_chain_state(w, chain, what)
        finally:
            w.close()


# ---------------------------------------------------------------------------------------------
# d. look-back repair through a far-off slot
# ---------------------------------------------------------------------------------------------

N_LOOKBACK = 300_000


@pytest.mark.parametrize("with_tx", [False, True], ids=["emit", "emit_tx"])
def test_lookback_repairs_the_saved_slot(gpu_worker_factory, monkeypatch, with_tx):
    """Every FWD4_HIT packet of a pair-sequence batch goes to one destination, the L1 entry at
    that address starts with a MAC the table contradicts, and every look-back that meets an
    unpublished chunk defers (spin 0): the last workgroup's repair rewrites records through the
    slot the wave saved, which differs from the packet's index by up to 63 in most groups.  One
    packet in the middle of the batch goes to another entry: the candidates before it take the
    starting entry's MAC, those after it the table's."""
    _mode(monkeypatch, "default")
    monkeypatch.setenv("UPE_GPU_LB_SPIN", "0")
    monkeypatch.setenv("UPE_GPU_NOLB", "0")
    t = ec.table(8)
    kinds = np.resize(ec.kinds_of(ec.pair_mask()), N_LOOKBACK)
    other = int(np.nonzero(kinds[150_001:] == ec.FWD4_HIT)[0][0]) + 150_001
    b = ec.build(kinds, "look-back", one_dst4=True, other_at=other)
    wl = ec.workload(b, t)
    l1 = synth.l1_zero()
    l1["last_arp_ip"] = int(ec.HIT4[0])
    l1["last_arp_mac"] = np.frombuffer(bytes.fromhex("0badc0ffee01"), np.uint8)
    wl.l1 = l1
    e = ec.expected(wl)
    aimed = np.nonzero(b.kinds == ec.FWD4_HIT)[0]
    stale = (e.records[aimed, :6] == l1["last_arp_mac"][0]).all(axis=1)
    assert stale[aimed < other].all() and not stale[aimed >= other].any()
    assert (np.abs(e.slots[aimed] - aimed) > 8).mean() > 0.25   # the saved slot is far from i
    w = _open(gpu_worker_factory, t, False, l1)
    try:
        info = _launch(w, b, e, with_tx, f"look-back tx={with_tx}", l1=l1)
    finally:
        w.close()
    print(f"look-back tx={with_tx}: deferred {info['deferred']}, grid {info['grid']}")
    assert not info["variant"] & gpu.VAR_NOLB, info
    assert info["deferred"] > 0, info


# ---------------------------------------------------------------------------------------------
# e. upe_gpu_compact on hand-made verdict words
# ---------------------------------------------------------------------------------------------

BLOCK = 4096   # kCompactBlock


def _block_patterns() -> dict:
    k = np.arange(BLOCK)
    rng = np.random.default_rng(31)
    return {"empty": k < 0, "full": k >= 0, "first": k == 0, "last": k == BLOCK - 1,
            "one_per_step": k % 256 == (k // 256 * 37) % 256, "seeded": rng.random(BLOCK) < 0.3}


def _block_pairs() -> np.ndarray:
    """Blocks in an order in which every ordered pair of patterns occurs as neighbours."""
    p = _block_patterns()
    names = list(p)
    return np.concatenate([p[names[v]] for v in ec.euler_circuit(len(names))])


def _words(match: np.ndarray, code: int, seed: int) -> np.ndarray:
    """Verdict words: `code` where match, another code elsewhere, all 28 upper bits set at random
    (some all ones, some all zero): only the code may be read."""
    rng = np.random.default_rng([37, seed])
    n = len(match)
    other = (code + 1 + rng.integers(0, 6, size=n)) % 7
    upper = rng.integers(0, 1 << 28, size=n, dtype=np.uint32)
    sel = rng.integers(0, 4, size=n)
    upper = np.where(sel == 0, (1 << 28) - 1, np.where(sel == 1, 0, upper)).astype(np.uint32)
    return (np.where(match, code, other).astype(np.uint32) | (upper << np.uint32(4))).astype(np.uint32)


def _compact_cases():
    pairs = _block_pairs()
    cases = [("pairs", pairs)]
    rng = np.random.default_rng(41)
    for n in (1, 255, 256, 257, 4095, 4096, 4097):
        cases.append((f"n{n}", rng.random(n) < 0.5))
        cases.append((f"n{n}:last", np.arange(n) == n - 1))
    big = 257 * BLOCK + 1            # 258 blocks: the prefix loop's second stride
    m = rng.random(big) < 0.01
    m[-1] = True
    cases.append(("second_stride", m))
    lone = np.zeros(big, bool)
    lone[-1] = True
    cases.append(("lone_last", lone))
    return cases


def _compact(w, d, words, code):
    n = len(words)
    v = d.put(words)
    index = d.poison(4 * (n + ec.CANARY))
    count = d.poison(8)
    w.compact(v, n, code, index, count)
    return (d.get(index, n + ec.CANARY, np.uint32), int(d.get(count, 1, np.uint64)[0]))


def test_compact_on_chosen_words(gpu_worker_factory):
    w = gpu_worker_factory(1024)
    t0 = time.perf_counter()
    try:
        for name, match in _compact_cases():
            # every code over the pair sequence and the small sizes, two over the 1M-word cases
            codes = range(7) if len(match) <= len(_block_pairs()) else (V_FWD, 0)
            for code in codes:
                words = _words(match, code, len(match) + code)
                want = np.nonzero(match)[0]
                assert np.array_equal(want, np.nonzero((words & 0xF) == code)[0])
                d = Dev(w)
                try:
                    index, count = _compact(w, d, words, code)
                    what = f"compact {name} code {code}"
                    assert count == len(want), f"{what}: count {count}, want {len(want)}"
                    bad = np.nonzero(index[:count] != want)[0]
                    assert bad.size == 0, (f"{what}: entry {int(bad[0])} is {int(index[bad[0]])}, "
                                           f"want {int(want[bad[0]])}")
                    assert (index[count:] == ec.POISON32).all(), f"{what}: written past the count"
                    if name == "pairs" and code == V_FWD:
                        # a code that never occurs: count 0, the index array untouched
                        for absent in (7, 15):
                            index, count = _compact(w, d, words, absent)
                            assert count == 0 and (index == ec.POISON32).all(), absent
                finally:
                    d.free()
    finally:
        w.close()
    print(f"compact: {time.perf_counter() - t0:.2f} s")
