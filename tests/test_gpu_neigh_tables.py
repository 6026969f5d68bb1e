"""Adversarial neighbour tables through every device lookup path, against the oracle bit for bit.

The classify kernels look a destination up in five places (upe_gpu.hip: arp_lookup_lds,
ndp_lookup_lds, the mixed-family neigh_lookup that reads the index from memory, and arp_lookup /
ndp_lookup of the L1 agreement check).  The tables of tests/neigh_cases.py — entries no probe
reaches, an address in two slots, stale addresses in invalid slots, chains that wrap, addresses of
one fold_v6 or one home slot, 0.0.0.0 and :: as entries and as destinations — run here small (both
indexes staged in LDS), embedded in 8192-slot tables (read from memory), one family each way, on
the two sides of the staging threshold, through every launch form, under every rule matcher (which
moves the indexes' place in the LDS carve-up), from starting L1 entries that disagree with the
table, and across a load that fails.  tests/test_neigh_cases.py pins, on the CPU, that every batch
reaches what its table is named for, and the oracle runs compared here are the ones it checked.
Verdict words, frames, counters, rule_stats and L1 must be equal.
"""
from __future__ import annotations

import numpy as np
import pytest

import neigh_cases as nc
import oracle
from test_gpu_mapped import _mapped_run
from test_gpu_parity import _assert_same
from test_gpu_rss_egress import _expected_hashes
from test_gpu_rule_tables import SMALL as SMALL_RULES, _set_mode
from test_neigh_cases import L1_STARTS, as_ref, l1_workload, oracle_of, workload
from upe_amd import gpu
from upe_amd.layout import V_FWD

pytestmark = pytest.mark.gpu

VAR_LEAN = 4   # upe_launch_info_t.variant bit 2: every non-empty neighbour index is staged in LDS
COMBINED, TWIN = "embed:combo", "combo"   # one workload for the launch forms, and its staged twin


def _classify(factory, wl, emit, l1=None):
    """One batch on a fresh context: (outputs, launch variant, rule index kind, tree nodes)."""
    w = factory(wl.capacity)
    try:
        w.configure(wl)
        if l1 is not None:
            w.set_l1(l1)
        got = gpu.run_workload(wl, worker=w, emit=emit)
        return (got, int(w.launch_info()["variant"]), w.rule_index_kind(),
                int(w.rule_index_info()["nodes"]))
    finally:
        w.close()


def _staged(name):
    """Whether every non-empty index of the case is staged (2048 slots at most), by the case's
    construction: the small tables and the boundary pair's lower side are, nothing else is."""
    if name.startswith("boundary:"):
        return name.endswith(":n")
    return name in nc.SMALL_CASES


@pytest.mark.parametrize("emit", [False, True], ids=["inplace", "emit"])
@pytest.mark.parametrize("name", nc.SMALL_CASES + nc.MEMORY_CASES + nc.BOUNDARY_CASES)
def test_table(gpu_worker_factory, monkeypatch, name, emit):
    _set_mode(monkeypatch, "default")
    got, variant, kind, _ = _classify(gpu_worker_factory, workload(name), emit)
    what = f"{name} emit={emit} variant {variant:#x}"
    print(what)
    assert kind == 0 and not variant & gpu.VAR_SCAN, what   # 8 rules: the small-table scan
    # staged or not: the boundary pair (1638 and 1639 reachable entries) straddles the bit
    assert bool(variant & VAR_LEAN) == _staged(name), what
    _assert_same(got, as_ref(oracle_of(name)), what)


@pytest.mark.parametrize("emit", [False, True], ids=["inplace", "emit"])
@pytest.mark.parametrize("name", nc.SPLIT_CASES)
def test_one_family_in_memory(gpu_worker_factory, monkeypatch, name, emit):
    """ARP in memory and NDP staged, and the reverse (both in memory: test_table's embed: cases):
    in a mixed wave one family's lanes take neigh_lookup and the other's the LDS lookup."""
    _set_mode(monkeypatch, "default")
    got, variant, _, _ = _classify(gpu_worker_factory, workload(name), emit)
    what = f"{name} emit={emit} variant {variant:#x}"
    assert not variant & VAR_LEAN, what
    _assert_same(got, as_ref(oracle_of(name)), what)


# ---------------------------------------------------------------------------------------------
# every launch form
# ---------------------------------------------------------------------------------------------

FORMS = ("rss", "emit_tx", "mapped", "mapped_emit", "host", "host_emit")


@pytest.mark.parametrize("form", FORMS)
def test_launch_forms(gpu_worker_factory, monkeypatch, form):
    _set_mode(monkeypatch, "default")
    wl, ref = workload(COMBINED), as_ref(oracle_of(COMBINED))
    n = wl.n
    chunked = False
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        if form == "rss":
            b = gpu.DeviceBatch(w, wl.frames, wl.desc)
            fh = w.malloc(4 * n)
            w.process_rss(b.frames, b.desc, b.verdict, fh, n)
            frames, verdict = b.fetch()
            hashes = np.zeros(n, np.uint32)
            w.d2h(hashes, fh)
            w.sync()
            w.free(fh)
            b.free()
            assert not w.launch_info()["variant"] & VAR_LEAN   # the hash keeps it off the lean kernel
            bad = np.nonzero(hashes != _expected_hashes(wl))[0]
            assert bad.size == 0, f"{bad.size} flow hashes differ, first {bad[:8].tolist()}"
        elif form == "emit_tx":
            b = gpu.DeviceBatch(w, wl.frames, wl.desc)
            b.hdr = w.malloc(16 * n)
            groups = (n + 63) // 64
            tx, cnt = w.malloc(4 * n), w.malloc(4 * groups)
            w.process_emit_tx(b.frames, b.desc, b.verdict, b.hdr, tx, cnt, n)
            rec = b.fetch_hdr()
            frames, verdict = b.fetch()
            got_tx, got_cnt = np.zeros(n, np.uint32), np.zeros(groups, np.uint32)
            w.d2h(got_tx, tx)
            w.d2h(got_cnt, cnt)
            w.sync()
            w.free(tx)
            w.free(cnt)
            b.free()
            assert w.launch_info()["variant"] & gpu.VAR_TX == gpu.VAR_TX
            frames = gpu.hdr_apply(frames, wl.desc, rec)
            lst = np.concatenate([got_tx[64 * g:64 * g + int(got_cnt[g])] for g in range(groups)])
            want = np.nonzero((ref["verdict"] & 0xF) == V_FWD)[0]
            assert np.array_equal(lst.astype(np.int64), want), "egress list"
        elif form.startswith("mapped"):
            frames, verdict, _, _, _ = _mapped_run(w, wl, form == "mapped_emit")
        else:
            # chunks of 1024: five launches, each starting from the L1 state the one before left
            chunked = True
            frames = wl.frames.copy()
            verdict = np.zeros(n, np.uint32)
            if form == "host":
                w.process_host(frames, wl.desc, verdict, 1024)
            else:
                rec = np.zeros((n, 16), np.uint8)
                w.process_host_emit(frames, wl.desc, verdict, rec, 1024, 0)
            assert w.launch_info()["launches"] >= 5
        counters, stats = w.get_stats()
        l1 = w.get_l1()
    finally:
        w.close()
    _assert_same((frames, verdict, counters, stats, l1), ref, form, batch_relative=chunked)


# ---------------------------------------------------------------------------------------------
# every rule matcher: the indexes' place in the LDS carve-up moves
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["scan", "tree", "tree-memory", "tss", "tss-unstaged"])
@pytest.mark.parametrize("n_rules", [200, 5000])
@pytest.mark.parametrize("name", [COMBINED, TWIN])
def test_rule_modes(gpu_worker_factory, monkeypatch, name, n_rules, mode):
    """plan_lds hands LDS out in the order bins, ARP index, NDP index, fingerprints, tree, family
    lists: with ~200 and ~5000 rules under each forced matcher the neighbour arrays sit behind
    bins of another size (or none) and in front of other neighbours."""
    _set_mode(monkeypatch, mode)
    wl = workload(name, n_rules)
    assert n_rules >= SMALL_RULES
    got, variant, kind, nodes = _classify(gpu_worker_factory, wl, emit=False)
    scan = variant & gpu.VAR_SCAN
    what = f"{name} {n_rules} rules {mode}: kind {kind}, variant {variant:#x}"
    print(what)
    if mode.startswith("tss"):
        assert kind == 1 and scan == 0, what
    elif mode == "scan":
        assert kind == 0 and scan in (gpu.VAR_FAM, gpu.VAR_GLB), what
    else:
        assert nodes > 0 and kind == 2 and scan == gpu.VAR_TREE, what
    _assert_same(got, as_ref(oracle_of(name, n_rules)), what)


# ---------------------------------------------------------------------------------------------
# starting L1 entries that the table contradicts, or never consults
# ---------------------------------------------------------------------------------------------

_L1_ORACLE: dict = {}


def _l1_oracle(name, which):
    """The oracle's two batches from the starting state, the second continued from the first."""
    if (name, which) not in _L1_ORACLE:
        wl, l1 = l1_workload(name, which)
        r1 = oracle.run_restated(wl, l1=l1)
        r2 = oracle.run_restated(wl, l1=r1.l1, counters=r1.counters, rule_stats=r1.rule_stats)
        _L1_ORACLE[name, which] = (r1, r2)
    return _L1_ORACLE[name, which]


@pytest.mark.parametrize("spin", [None, "0"], ids=["spin", "deferred"])
@pytest.mark.parametrize("which", L1_STARTS)
@pytest.mark.parametrize("name", [TWIN, COMBINED])
def test_l1_interplay(gpu_worker_factory, monkeypatch, name, which, spin):
    """Two batches on one context (the first rewritten in place, the second in emit mode), L1,
    counters and stats carried over.  The starting L1 names (a) a duplicated address with the
    second slot's MAC, (b) a hidden entry's address and MAC, (c) 0.0.0.0 with a MAC while the
    table holds 0.0.0.0, (d) nothing (calloc) while the table holds ::; a whole wave of packets to
    the named address leads the batch.  Once as it comes, once with every look-back deferred to
    the repair pass (UPE_GPU_LB_SPIN=0)."""
    _set_mode(monkeypatch, "default")
    if spin is None:
        monkeypatch.delenv("UPE_GPU_LB_SPIN", raising=False)
    else:
        monkeypatch.setenv("UPE_GPU_LB_SPIN", spin)
    wl, l1 = l1_workload(name, which)
    r1, r2 = _l1_oracle(name, which)
    w = gpu_worker_factory(wl.capacity)
    try:
        w.configure(wl)
        w.set_l1(l1)
        got1 = gpu.run_workload(wl, worker=w, emit=False)
        v1 = int(w.launch_info()["variant"])
        got2 = gpu.run_workload(wl, worker=w, emit=True)
    finally:
        w.close()
    what = f"{name} {which} spin={spin}"
    _assert_same(got1, as_ref(r1), what + " batch 1")
    _assert_same(got2, as_ref(r2), what + " batch 2")
    if which in ("dup_second", "hidden"):
        assert not v1 & gpu.VAR_NOLB, what + ": the first batch ran without look-back"


# ---------------------------------------------------------------------------------------------
# a load that fails
# ---------------------------------------------------------------------------------------------

def test_failed_load_keeps_the_snapshot(gpu_worker_factory, monkeypatch):
    """upe_gpu_load_neigh is all or nothing (include/upe_gpu.h).  Four reachable NDP addresses of
    one fold_v6 share their three candidate slots and cannot be placed: the call returns -1 on
    the host, before any upload, and the context goes on with the tables it had — the valid ARP
    table of the failed call is not installed either.  With three of the four the same call
    succeeds (so the four did share a fold: had they not, the first call would have succeeded)."""
    _set_mode(monkeypatch, "default")
    wl0 = workload(TWIN)
    r0 = oracle_of(TWIN)
    new = nc.Case("after the load", "wrap", "one_fold")
    arp_new = nc.table("arp", "wrap")
    four, three = nc._one_fold("ndp", 4), nc.table("ndp", "one_fold")
    assert len(nc.anatomy(four)["reachable"]) == 4 and len(nc.anatomy(three)["reachable"]) == 3
    assert not np.array_equal(arp_new, wl0.arp[:len(arp_new)])
    wl2 = nc.traffic(new)
    # the oracle, continued: wl0 twice under T0, then wl2 under the new tables
    r1 = oracle.run_restated(wl0, l1=r0.l1, counters=r0.counters, rule_stats=r0.rule_stats)
    r2 = oracle.run_restated(wl2, l1=r1.l1, counters=r1.counters, rule_stats=r1.rule_stats)
    w = gpu_worker_factory(wl0.capacity)
    try:
        w.configure(wl0)
        _assert_same(gpu.run_workload(wl0, worker=w), as_ref(r0), "under T0")
        a, b = np.ascontiguousarray(arp_new), np.ascontiguousarray(four)
        rc = gpu.LIB.upe_gpu_load_neigh(w._ctx, a.ctypes.data, len(a), b.ctypes.data, len(b))
        msg = gpu.LIB.upe_gpu_last_error().decode()
        assert rc == -1 and "placement" in msg, (rc, msg)
        _assert_same(gpu.run_workload(wl0, worker=w, emit=True), as_ref(r1),
                     "after the failed load: still T0, both families")
        w.load_neigh(arp_new, three)
        _assert_same(gpu.run_workload(wl2, worker=w), as_ref(r2), "under the new tables")
    finally:
        w.close()
