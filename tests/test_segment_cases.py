"""CPU: the batches of tests/segment_cases.py do what they are named for, before any GPU sees
them (tests/test_gpu_segment_cases.py runs them through upe_gpu_process_segmented and
upe_gpu_process_segmented_resident).

For every case: upe_ctrl_writes_host finds the stated marked packets and records at the stated
positions; neigh.patch / upe_neigh_apply_writes, record by record, give the stated (writes,
patched, rebuilds); the restated worker with control replay (and the reference worker, where it is
built) leaves every named probe with the stated old / new / no MAC; at most half of a batch is
filler.  The oracle run the GPU tests compare with (segment_cases.oracle_run: the restated worker
segment by segment) equals the one-batch run everywhere but in UPE_VF_L1_INIT.
"""
from __future__ import annotations

import numpy as np
import pytest

import neigh_cases as nc
import oracle
import segment_cases as sc
from upe_amd import gpu, neigh
from upe_amd.layout import CW_ARP, V_FWD, VF_L1_INIT, VF_NEIGH_HIT, desc_offsets

KEEP = ["ip", "mac", "valid"]


def derived(wl, now=sc.NOW):
    """(writes, patched, rebuilds) numpy derives, as tests/test_gpu_segmented_resident._derived:
    neigh.patch record by record over the tables as the writes leave them.  Also the tables."""
    recs, _ = gpu.ctrl_writes_host(wl.frames, wl.desc)
    arp, ndp = wl.arp.copy(), wl.ndp.copy()
    patched = rebuilds = 0
    for j in range(len(recs)):
        if not len(arp if recs["kind"][j] == CW_ARP else ndp):
            continue
        if neigh.patch(arp, ndp, recs[j:j + 1])[3][1]:
            patched += 1
        else:
            rebuilds += 1
        assert gpu.neigh_apply_writes(arp, ndp, recs[j:j + 1], now) == 1
    return (patched + rebuilds, patched, rebuilds), arp, ndp


@pytest.mark.parametrize("name", sc.ALL)
def test_records_and_counts(name):
    c = sc.case(name)
    recs, info = gpu.ctrl_writes_host(c.wl.frames, c.wl.desc)
    assert int(info["ctrl"]) == c.expect[0] == len(c.cuts), name
    assert int(info["writes"]) == len(c.records) == len(recs), name
    assert recs["index"].tolist() == list(c.records), name
    assert set(c.records) <= set(c.cuts) and list(c.cuts) == sorted(set(c.cuts))
    got, arp, ndp = derived(c.wl)
    assert got == c.expect[1:], (name, got, c.expect)
    # every applied record carries the caller's timestamp; the oracle's tables are these
    r = sc.oracle_of(name)
    assert np.array_equal(arp[KEEP], r.arp[KEEP]) and np.array_equal(ndp[KEEP], r.ndp[KEEP]), name
    if c.expect[1]:
        assert (arp["update_at"] == sc.NOW).sum() + (ndp["update_at"] == sc.NOW).sum() > 0


@pytest.mark.parametrize("name", sc.ALL)
def test_filler_share(name):
    """The packets that are neither marked nor a probe of an address a control packet names are
    at most half of the batch, and 8 to about 2100 packets make a batch."""
    c = sc.case(name)
    n = c.wl.n
    assert c.filler == n - len(c.cuts) - len(c.probes)
    assert 2 * c.filler <= n, (name, c.filler, n)
    assert 8 <= n <= 2100 or name == "count:1", (name, n)
    assert not set(i for i, _, _ in c.probes) & set(c.cuts)


def _check_probes(c, r, what):
    offs = desc_offsets(c.wl.desc)
    for i, want, m in c.probes:
        o = int(offs[i])
        assert int(r.verdict[i]) & 0xF == V_FWD, (what, i)
        got = r.frames[o:o + 6].tobytes()
        if want == "none":
            assert not r.verdict[i] & VF_NEIGH_HIT and got == sc.UNTOUCHED, (what, i, got.hex())
        else:
            assert r.verdict[i] & VF_NEIGH_HIT and got == m, (what, i, want, got.hex(), m.hex())


@pytest.mark.parametrize("name", sc.ALL)
def test_probes_see_what_is_stated(name):
    """The restated worker with control replay, the same run segment by segment, and the
    reference worker where it is built and both families have a table: each named probe leaves
    with the stated MAC."""
    c = sc.case(name)
    whole = oracle.run_restated(c.wl, apply_control=True)
    _check_probes(c, whole, name + " restated")
    r = sc.oracle_of(name)
    _check_probes(c, r, name + " by segment")
    keep = ~np.uint32(VF_L1_INIT)
    assert np.array_equal(r.verdict & keep, whole.verdict & keep)
    assert np.array_equal(r.frames, whole.frames) and r.l1.tobytes() == whole.l1.tobytes()
    assert r.counters.tobytes() == whole.counters.tobytes()
    assert np.array_equal(r.rule_stats, whole.rule_stats)
    kinds = {want for _, want, _ in c.probes}
    if name.split(":")[1] not in ("only8", "both0"):
        assert "new" in kinds or name in ("norecord:all", "place:last:new", "place:last:held"), name
    # (a family without a table is this library's notion: the reference worker always has both,
    # and oracle/ref_harness.c gives it one slot where the capacity is 0, which then learns)
    if oracle.ref_available() and len(c.wl.arp) and len(c.wl.ndp):
        ref = oracle.run_reference(c.wl)
        _check_probes(c, ref, name + " reference")
        assert np.array_equal(ref.verdict, whole.verdict)
        assert np.array_equal(ref.frames, whole.frames)
        assert np.array_equal(ref.arp[KEEP], whole.arp[KEEP])
        assert np.array_equal(ref.ndp[KEEP], whole.ndp[KEEP])


@pytest.mark.parametrize("form", sc.FORMS)
def test_the_probe_before_keeps_the_old_answer(form):
    """place:*: a probe stands before and behind the control packet wherever the placement leaves
    room, the one before with the old answer; in place:middle the control packet's 64-packet
    group holds probes of both kinds."""
    for where in sc.PLACES:
        c = sc.case(f"place:{where}:{form}")
        first = c.cuts[0]
        pre = [w for i, w, _ in c.probes if i < first]
        post = [w for i, w, _ in c.probes if i > c.cuts[-1]]
        assert all(w == ("old" if form == "held" else "none") for w in pre), where
        assert all(w == "new" for w in post), where
        assert bool(pre) == (where not in ("first", "only8")), where
        assert bool(post) == (where not in ("last", "only8")), where
    c = sc.case(f"place:middle:{form}")
    group = [w for i, w, _ in c.probes if i // 64 == c.cuts[0] // 64]
    assert "new" in group and len(set(group)) == 2 and c.wl.n > 128
    assert sc.case(f"place:first:{form}").cuts == (0,)
    c = sc.case(f"place:last:{form}")
    assert c.cuts == (c.wl.n - 1,)
    assert sc.case(f"place:adjacent2:{form}").cuts == (2, 3)
    assert sc.case(f"place:adjacent3:{form}").cuts == (5, 6, 7)
    assert sc.case(f"place:only8:{form}").cuts == tuple(range(8))


def test_port_request_is_answered_in_place():
    """The record's MAC and address are gone from the frame after the batch (the reply carries
    the port's), so a record built after the rewrite would teach the port's own address."""
    c = sc.case("place:port:held")
    r = sc.oracle_of(c.name)
    k = c.cuts[0]
    o = int(desc_offsets(c.wl.desc)[k])
    assert r.verdict[k] & 0x60 == 0x60   # ARP_LEARN | ARP_REPLY
    assert c.wl.frames[o + 22:o + 28].tobytes() == sc.mac(0x11, 0)
    assert r.frames[o + 22:o + 28].tobytes() == bytes(c.wl.eth_addr)
    assert int.from_bytes(r.frames[o + 28:o + 32].tobytes(), "big") == c.wl.ip4_addr


@pytest.mark.parametrize("which", ["ns", "na", "arp"])
def test_norecord_cut_shows_in_l1_init(which):
    """The second packet of the flow carries UPE_VF_L1_INIT because the marked packet between the
    two cuts the batch (the flag is defined against the entry a segment starts from); with the
    marked packet taken out it does not.  The one-batch restatement (oracle.run_restated) has no
    cuts and never sets it here; segment_cases.oracle_run, which the GPU tests compare whole
    verdict words with, does."""
    c = sc.case(f"norecord:{which}")
    a, k, b = sc.flow_pair(c)
    assert k not in c.records or which == "arp"
    r = sc.oracle_of(c.name)
    assert r.verdict[b] & VF_L1_INIT and not r.verdict[a] & VF_L1_INIT
    d = sc.without(c, k)
    rd = sc.oracle_run(d)
    assert not rd.verdict[b - 1] & VF_L1_INIT
    assert (rd.verdict[b - 1] | VF_L1_INIT) == r.verdict[b]
    assert not oracle.run_restated(c.wl, apply_control=True).verdict[b] & VF_L1_INIT


def test_norecord_all_and_notable_write_what_is_stated():
    c = sc.case("norecord:all")
    assert c.expect == (4, 0, 0, 0) and c.records == ()
    assert sc.case("notable:both0").expect == (4, 0, 0, 0)
    assert len(sc.case("notable:both0").records) == 4
    for name in ("notable:arp0", "notable:ndp0"):
        c = sc.case(name)
        recs, _ = gpu.ctrl_writes_host(c.wl.frames, c.wl.desc)
        assert c.expect == (4, 2, 1, 1) and sorted(set(recs["kind"].tolist())) == [4, 6]
        assert (len(c.wl.arp) == 0) == (name == "notable:arp0")
        assert (len(c.wl.ndp) == 0) == (name == "notable:ndp0")
    assert len(sc.case("norecord:arp").wl.arp) == 0


def test_count_cases():
    for n in sc.COUNTS:
        c = sc.case(f"count:{n}")
        assert c.expect == (n, n, n, 0) and c.wl.n == 2 * n and c.filler == 0
    c = sc.case("count:1025:alt")
    recs, info = gpu.ctrl_writes_host(c.wl.frames, c.wl.desc)
    assert len(recs) == int(info["writes"]) == 1025 and c.expect == (1025, 1025, 513, 512)
    assert len(sc.case("count:1025").records) == 1025
    # the MAC names the rank: records and probes alternate, record j at 2 j
    assert recs["index"].tolist() == list(range(0, 2050, 2))
    assert all(bytes(recs["mac"][j]) == sc.mac(0xC0, j) for j in (0, 1, 1023, 1024))
    # the new addresses fit
    r = sc.oracle_of(c.name)
    assert int(r.arp["valid"].sum()) == 16 + 512


@pytest.mark.parametrize("name", [n for n in sc.ALL if n.startswith("tables:")])
def test_tables_start_from_the_named_anatomy(name):
    c = sc.case(name)
    small = c.base.split(":")[-1]
    for fam, t in (("arp", c.wl.arp), ("ndp", c.wl.ndp)):
        assert np.array_equal(t, nc.table(fam, c.base))
        an = nc.anatomy(nc.table(fam, small))
        if small == "hidden":
            assert an["hidden"] and an["stale"]
        elif small == "dup":
            assert len(an["dup"]) == 2
        elif small == "stale_head":
            assert an["stale"] and not an["hidden"]
        elif small == "wrap":
            t16 = nc.table(fam, small)
            assert t16["valid"][[14, 15, 0, 1]].all()
        else:
            assert nc.ZERO[fam] in an["reachable"]
        # the big table holds the small one's addresses where the same probes find them
        big = nc.anatomy(t) if c.base.startswith("embed:") else an
        for k in ("hidden", "stale", "dup"):
            assert set(an[k]) <= set(big[k]), (name, fam, k)
        targets = sc.table_targets(fam, small)
        assert len({a for a, _ in targets}) == len(targets)
        assert nc.Probe(t).slot(targets[-1][0]) < 0 and targets[-1][0] not in nc.stored(t)
    if c.base.startswith("embed:"):
        assert len(c.wl.arp) == nc.BIG
    # the second round refreshes everything the first taught
    assert c.expect[2] > c.expect[3] > 0 and c.expect[1] == len(c.records) == len(c.probes)


@pytest.mark.parametrize("size", ["staged", "memory"])
@pytest.mark.parametrize("form", sc.FORMS)
def test_place_tables_around_the_staging_threshold(size, form):
    """place:adjacent3 over 4096-slot tables: at most neigh_cases.BOUNDARY_N reachable entries
    before and after the batch (an index of 2048 slots, staged in LDS), or more from the start
    (4096 slots, read from memory) — by the compiled snapshot's own size."""
    c = sc.case(f"place:adjacent3:{form}:{size}", 200)
    small = sc.case(f"place:adjacent3:{form}")
    assert c.expect == small.expect and c.cuts == small.cuts and c.probes == small.probes
    r = sc.oracle_of(c.name, 200)
    _check_probes(c, r, c.name)
    for arp, ndp in ((c.wl.arp, c.wl.ndp), (r.arp, r.ndp)):
        image = gpu.NeighImage(arp, ndp)
        info = image.read()[0]
        image.free()
        for fam, t in (("arp", arp), ("ndp", ndp)):
            reach = len(nc.anatomy(t)["reachable"])
            assert (reach <= nc.BOUNDARY_N) == (size == "staged"), (fam, reach)
            assert int(info[fam + "_bits"]) == (11 if size == "staged" else 12), (fam, info)
