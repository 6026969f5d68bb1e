"""CPU: the adversarial neighbour tables of tests/neigh_cases.py do what they are named for.

For every case the C restatement equals the reference worker (where it is built), and both equal
a third statement of the neighbour step written here in Python (the reference's probe over the
slot array plus the one-entry L1 cache, src/worker.c:186-195, 218-225) on every forwarded packet:
whether UPE_VF_NEIGH_HIT is set and which destination MAC the frame carries.  On top of that, the
oracle's own outputs show each case's point: packets to hidden and stale addresses leave
unflagged, a duplicated address answers with its first slot's MAC, a batch ending on 0.0.0.0
leaves last_arp_ip = 0 with that entry's MAC, :: is answered by the calloc'd L1 entry until
another IPv6 packet hits the table.  tests/test_gpu_neigh_tables.py then compares the kernels
with the same oracle runs, so it cannot pass on a batch that misses the case.
"""
from __future__ import annotations

import numpy as np
import pytest

import neigh_cases as nc
import oracle
from keyframes import RUN
from upe_amd import synth
from upe_amd.layout import (L1_DTYPE, V_DROP_ACTION, V_DROP_PARSE, V_DROP_RULE, V_DROP_TTL, V_FWD,
                            VF_NEIGH_HIT, desc_offsets)

ALL_CASES = nc.SMALL_CASES + nc.MEMORY_CASES + nc.BOUNDARY_CASES + nc.SPLIT_CASES
_WL: dict = {}
_ORACLE: dict = {}


def workload(name, n_rules=8):
    if (name, n_rules) not in _WL:
        _WL[name, n_rules] = nc.traffic(nc.case(name), n_rules=n_rules)
    return _WL[name, n_rules]


def as_ref(r):
    return {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
            "rule_stats": r.rule_stats, "l1": r.l1}


def check_against_reference(wl, r, what, l1=None):
    """The restatement's run `r` of `wl` equals the reference worker's, where it is built."""
    if not oracle.ref_available():
        return
    ref = oracle.run_reference(wl, l1=l1)
    assert np.array_equal(ref.verdict, r.verdict), f"{what}: restatement vs worker"
    assert np.array_equal(ref.frames, r.frames), what
    assert ref.counters.tobytes() == r.counters.tobytes(), what
    assert np.array_equal(ref.rule_stats, r.rule_stats), what
    assert ref.l1.tobytes() == r.l1.tobytes(), what


def oracle_of(name, n_rules=8):
    """One restated run per workload, shared by the CPU and GPU tests and left unchanged."""
    if (name, n_rules) not in _ORACLE:
        wl = workload(name, n_rules)
        r = oracle.run_restated(wl)
        check_against_reference(wl, r, name)
        _ORACLE[name, n_rules] = r
    return _ORACLE[name, n_rules]


def neighbour_model(wl, verdict, l1=None):
    """Per packet, for the forwarded ones: (answered, MAC, "l1" | "table" | None) by the
    reference's neighbour step restated in Python over wl's slot arrays, from L1 state `l1`.
    Also returns the final L1 state."""
    fams, dsts = nc.destinations(wl)
    l1 = (wl.l1 if l1 is None else l1).copy()
    probe = {4: nc.Probe(wl.arp), 6: nc.Probe(wl.ndp)}
    last = {4: (int(l1["last_arp_ip"][0]), l1["last_arp_mac"][0].tobytes()),
            6: (l1["last_ndp_ip"][0].tobytes(), l1["last_ndp_mac"][0].tobytes())}
    out = [None] * wl.n
    for i in np.nonzero((verdict & 0xF) == V_FWD)[0].tolist():
        f, d = int(fams[i]), dsts[i]
        if d == last[f][0] and (f == 6 or d != 0):   # (0.0.0.0 is never asked of the L1 entry)
            out[i] = (True, last[f][1], "l1")
            continue
        mac = probe[f].mac(d)
        if mac is None:
            out[i] = (False, None, None)
        else:
            last[f] = (d, mac)
            out[i] = (True, mac, "table")
    l1["last_arp_ip"] = last[4][0]
    l1["last_arp_mac"] = np.frombuffer(last[4][1], np.uint8)
    l1["last_ndp_ip"] = np.frombuffer(last[6][0], np.uint8)
    l1["last_ndp_mac"] = np.frombuffer(last[6][1], np.uint8)
    return out, l1


def check_model(wl, r, what, l1=None):
    """The oracle's flags, destination MACs and final L1 equal the Python model's."""
    model, end = neighbour_model(wl, r.verdict, l1)
    offs = desc_offsets(wl.desc)
    for i, m in enumerate(model):
        if m is None:
            continue
        o = int(offs[i])
        assert bool(r.verdict[i] & VF_NEIGH_HIT) == m[0], f"{what}: packet {i} {m}"
        want = m[1] if m[0] else wl.frames[o:o + 6].tobytes()   # a miss leaves the MACs alone
        assert r.frames[o:o + 6].tobytes() == want, f"{what}: packet {i} destination MAC"
        if not m[0]:
            assert r.frames[o + 6:o + 12].tobytes() == wl.frames[o + 6:o + 12].tobytes()
    assert end.tobytes() == r.l1.tobytes(), f"{what}: final L1"
    return model


# ---------------------------------------------------------------------------------------------
# the helpers
# ---------------------------------------------------------------------------------------------

def test_helpers_mirror_the_sources():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        for cap in (1, 16, 8192):
            assert nc.home("ndp", k, cap) == synth.ndp_hash(k, cap)
    assert (0x9E3779B1 * nc.FOLD_INV) & nc.M32 == 1
    a = nc.homed("ndp", 16, 3, 77)
    b = nc.same_fold(a, 1, 2, 3)
    assert b != a and nc.fold_v6(nc.words("ndp", b)) == nc.fold_v6(nc.words("ndp", a))
    # fold_v6 as upe_dev.h writes it, on a value worked by hand: words (1, 0, 0, 0) and (0, 0, 0, 1)
    assert nc.fold_v6((1, 0, 0, 0)) == 0x9E3779B1 and nc.fold_v6((0, 0, 0, 1)) == 0x27D4EB2F
    for fam in ("arp", "ndp"):
        for cap, h in ((1, 0), (8, 5), (16, 14), (1024, 700), (32, 3)):
            k = nc.homed(fam, cap, h, 9)
            assert nc.home(fam, k, cap) == h
            assert nc.home(fam, k, nc.BIG) == (h if h < cap // 2 else nc.BIG - cap + h)
        assert len({nc.homed(fam, 16, 2, t) for t in range(50)}) == 50
    # insert is the reference's update, as synth's table builders restate it
    ips = [int(x) for x in rng.integers(1, 1 << 32, size=40)]
    t = nc.new_table("arp", 64)
    for ip in ips:
        nc.insert(t, ip)
    want = synth.arp_table(64, [(ip, b"\0" * 6) for ip in ips])
    assert np.array_equal(t["ip"], want["ip"]) and np.array_equal(t["valid"], want["valid"])
    v6 = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(40)]
    t = nc.new_table("ndp", 64)
    for ip in v6:
        nc.insert(t, ip)
    want = synth.ndp_table(64, [(ip, b"\0" * 6) for ip in v6])
    assert np.array_equal(t["ip"], want["ip"]) and np.array_equal(t["valid"], want["valid"])
    p = nc.Probe(t)
    lib = oracle.oracle_lib()
    mac = np.zeros(6, np.uint8)
    for ip in v6 + [bytes(16)]:
        buf = np.frombuffer(ip, np.uint8).copy()
        hit = lib.upe_ref_ndp_lookup(t.ctypes.data, len(t), buf.ctypes.data, mac.ctypes.data)
        assert hit == (p.mac(ip) is not None) and (not hit or mac.tobytes() == p.mac(ip))


@pytest.mark.parametrize("fam", ["arp", "ndp"])
def test_tables_have_their_shapes(fam):
    """What each table's name promises, by the reference's probe over the slot array."""
    an = {t: nc.anatomy(nc.table(fam, t)) for t in nc.FAMILY_TABLES if
          fam == "ndp" or t not in nc.NDP_ONLY}
    zero = nc.ZERO[fam]
    assert len(nc.table(fam, "cap0")) == 0 and not nc.stored(nc.table(fam, "cap1_empty"))
    assert len(an["cap1_full"]["reachable"]) == 1
    for t, cap in (("full8", 8), ("full1024", 1024)):
        assert len(an[t]["reachable"]) == cap and not an[t]["hidden"]
    assert sorted(an["wrap"]["reachable"].values()) == [0, 1, 14, 15]
    assert an["hidden"]["hidden"] == [nc.homed(fam, 16, 2, 3)]
    assert an["hidden"]["stale"] == [nc.homed(fam, 16, 2, 2)]
    assert an["stale_head"]["stale"] == [nc.homed(fam, 16, 2, 1)]
    assert sorted(an["stale_head"]["reachable"].values()) == [3, 4]
    assert an["dup"]["dup"] == [nc.homed(fam, 16, 14, 5), nc.homed(fam, 16, 2, 2)]
    assert an["dup"]["reachable"][nc.homed(fam, 16, 2, 2)] == 3
    assert an["dup"]["reachable"][nc.homed(fam, 16, 14, 5)] == 15   # slot 0 holds the other copy
    assert an["key0"]["reachable"][zero] == 1 and zero not in nc.stored(nc.table(fam, "no_key0"))
    assert len(an["key0"]["reachable"]) == len(an["no_key0"]["reachable"]) + 1 == 4
    c = an["combo"]
    assert c["reachable"][zero] == 1 and len(c["hidden"]) == 1 and len(c["stale"]) == 1 and \
        [c["reachable"][k] for k in c["dup"]] == [31, 11] and len(c["reachable"]) == 8
    if fam == "ndp":
        keys = list(an["one_fold"]["reachable"])
        assert len(keys) == 3 and len({nc.fold_v6(nc.words("ndp", k)) for k in keys}) == 1
        assert sorted(an["one_home"]["reachable"].values()) == [2, 3, 4, 5, 6]
        assert len({nc.home("ndp", k, 16) for k in an["one_home"]["reachable"]}) == 1
    big = an["big4096"]
    assert len(big["reachable"]) > 2048 * 4 // 5 and len(big["hidden"]) > 20 and \
        len(big["stale"]) > 20 and len(big["dup"]) > 0
    for t, n in (("boundary_n", nc.BOUNDARY_N), ("boundary_n1", nc.BOUNDARY_N + 1)):
        assert len(an[t]["reachable"]) == n and not an[t]["hidden"] and not an[t]["stale"]
    # cuckoo3_place's starting size: the least 2^bits with 4 * 2^bits >= 5 n
    assert 4 * 2048 >= 5 * nc.BOUNDARY_N and 4 * 2048 < 5 * (nc.BOUNDARY_N + 1)
    assert 4 * 2048 >= 5 * 1024 > 4 * 1024


@pytest.mark.parametrize("fam", ["arp", "ndp"])
@pytest.mark.parametrize("name", nc.EMBEDDED)
def test_embed_keeps_the_case(fam, name):
    """embed leaves the case's slots byte for byte as they were, and every query answers as in
    the small table; with the fillers the index must pass 2048 slots."""
    if fam == "arp" and name in nc.NDP_ONLY:
        name = "dup"
    small, big = nc.table(fam, name), nc.table(fam, "embed:" + name)
    cap = len(small)
    assert len(big) == nc.BIG
    for s in range(cap):
        t = nc.embed_slot(cap, s)
        assert big[t:t + 1].tobytes() == small[s:s + 1].tobytes()   # (padding and all)
    fill = nc.fillers(fam)
    mine = np.zeros(nc.BIG, bool)
    mine[[nc.embed_slot(cap, s) for s in range(cap)]] = True
    assert np.array_equal(big[~mine], fill[~mine]) and int(fill["valid"].sum()) == nc.FILLERS
    ps, pb = nc.Probe(small), nc.Probe(big)
    filler_keys = set(nc.stored(fill))
    cs = nc.case("embed:" + name if not (fam == "arp" and name == "dup") else "embed:dup")
    fams, dsts = nc.destinations(workload(cs.name))
    asked = {d for f, d in zip(fams.tolist(), dsts) if f == (4 if fam == "arp" else 6)}
    own = set(nc.stored(small))
    assert own <= asked
    n = 0
    for d in asked - filler_keys:
        assert ps.mac(d) == pb.mac(d), f"{fam} {name}: {d!r} answers differently once embedded"
        n += 1
    assert n > 200
    assert len(nc.anatomy(big)["reachable"]) == nc.FILLERS + len(nc.anatomy(small)["reachable"])
    assert 5 * nc.FILLERS > 4 * 2048


# ---------------------------------------------------------------------------------------------
# the batches
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_CASES)
def test_case_reaches_its_point(name):
    wl = workload(name)
    r = oracle_of(name)
    cs = nc.case(name)
    assert wl.n == nc.N_PACKETS and len(wl.rules) == 8
    code = r.verdict & 0xF
    fwd = code == V_FWD
    flag = (r.verdict & VF_NEIGH_HIT) != 0
    model = check_model(wl, r, name)
    fams, dsts = nc.destinations(wl)
    offs = desc_offsets(wl.desc)
    # every outcome, and forwarded packets with and without the flag
    for c, least in ((V_DROP_PARSE, 6), (V_DROP_RULE, 100), (V_DROP_ACTION, 50), (V_DROP_TTL, 50)):
        assert (code == c).sum() >= least, (c, int((code == c).sum()))
    assert (fwd & flag).sum() > 8 and (fwd & ~flag).sum() > 200
    # waves of one family and waves of both, and both families in every mixed wave
    kinds = set()
    for s in range(0, wl.n - RUN + 1, RUN):
        kinds.add(tuple(sorted(set(fams[s:s + RUN].tolist()) - {0})))
    assert kinds >= {(4,), (6,), (4, 6)}
    # L1 hits as well as table hits, in both families where a table holds anything
    for f, fam in ((4, "arp"), (6, "ndp")):
        how = [m[2] for i, m in enumerate(model) if m is not None and fams[i] == f]
        an = nc.anatomy(cs.table(fam))
        # (a single reachable address is looked up once, the L1 entry answers from then on; two
        # are looked up as often as the traffic goes from one to the other)
        if an["reachable"]:
            least = 10 if len(an["reachable"]) > 2 else len(an["reachable"]) - 1
            assert how.count("table") > least and how.count("l1") > 10, (fam, len(how))
        to = lambda keys: np.array([fams[i] == f and dsts[i] in keys for i in range(wl.n)]) & fwd
        # every stored address of the case is a forwarded packet's destination
        sent = {dsts[i] for i in np.nonzero(fwd & (fams == f))[0]}
        assert set(cs.own(fam)) <= sent, f"{fam}: {len(set(cs.own(fam)) - sent)} own addresses unsent"
        # hidden and stale addresses: forwarded, never flagged (nothing ever puts one into L1)
        lost = set(an["hidden"]) | set(an["stale"])
        if lost:
            m = to(lost)
            assert m.sum() >= min(len(lost), 100) and not (m & flag).any(), fam
            for i in np.nonzero(m)[0]:
                o = int(offs[i])
                assert r.frames[o:o + 12].tobytes() == wl.frames[o:o + 12].tobytes()
        # a duplicated address: the first slot's MAC
        p = nc.Probe(cs.table(fam))
        for k in an["dup"][:8]:
            m = to({k})
            first = an["reachable"][k]
            others = [s for s in range(p.cap) if p.valid[s] and p.keys[s] == k and s != first]
            assert others and p.macs[others[0]] != p.macs[first]
            if cs.own(fam) and k in cs.own(fam):
                assert m.sum() > 0
            for i in np.nonzero(m)[0]:
                assert r.frames[int(offs[i]):int(offs[i]) + 6].tobytes() == p.macs[first]
    # 0.0.0.0: the batch ends on it; where the table holds it the L1 entry ends as (0, its MAC)
    assert fams[wl.n - 1] == 4 and dsts[wl.n - 1] == 0 and fwd[wl.n - 1]
    an4 = nc.anatomy(cs.arp)
    to0 = fwd & (fams == 4) & np.array([d == 0 for d in dsts])
    assert to0.sum() >= 8
    if 0 in an4["reachable"]:
        mac = nc.Probe(cs.arp).macs[an4["reachable"][0]]
        assert int(r.l1["last_arp_ip"][0]) == 0 and r.l1["last_arp_mac"][0].tobytes() == mac
        assert flag[to0].all()
        assert all(model[i][2] == "table" for i in np.nonzero(to0)[0])   # never from L1
    else:
        assert not flag[to0].any()
    # ::, from the calloc'd L1 entry until another IPv6 packet hits the table
    to00 = fwd & (fams == 6) & np.array([d == bytes(16) for d in dsts])
    hits6 = [i for i, m in enumerate(model) if m is not None and fams[i] == 6 and m[2] == "table"
             and dsts[i] != bytes(16)]
    before = to00 & (np.arange(wl.n) < (hits6[0] if hits6 else wl.n))
    assert before.sum() >= 1 and to00.sum() >= 8
    for i in np.nonzero(before)[0]:
        assert flag[i] and r.frames[int(offs[i]):int(offs[i]) + 6].tobytes() == bytes(6)
        assert model[i][2] == "l1"
    later = to00 & ~before
    if hits6:
        assert later.sum() >= 1
        an6 = nc.anatomy(cs.ndp)
        if bytes(16) in an6["reachable"]:
            assert flag[later].all()
        else:
            assert not flag[later].any()


@pytest.mark.parametrize("n_rules", [200, 5000])
@pytest.mark.parametrize("name", ["embed:combo", "combo"])
def test_larger_rule_tables_change_nothing_but_the_walk(name, n_rules):
    """The fill rules match none of the traffic: the same packets forward, deeper in the table."""
    wl, r = workload(name, n_rules), oracle_of(name, n_rules)
    assert len(wl.rules) == n_rules
    check_model(wl, r, f"{name} {n_rules} rules")
    idx = (r.verdict >> 8).astype(np.int64) - 1
    fwd = (r.verdict & 0xF) == V_FWD
    assert set(idx[fwd].tolist()) == {n_rules - 2, n_rules - 1}
    assert set(idx[(r.verdict & 0xF) == V_DROP_RULE].tolist()) == {0, 1}


L1_STARTS = ("dup_second", "hidden", "zero_arp", "calloc_zero6")


def l1_start(which, cs):
    """The starting L1 states of the interplay tests (tests/test_gpu_neigh_tables.py)."""
    l1 = np.zeros(1, L1_DTYPE)
    for fam, ipf, macf in (("arp", "last_arp_ip", "last_arp_mac"),
                           ("ndp", "last_ndp_ip", "last_ndp_mac")):
        t = cs.table(fam)
        an, p = nc.anatomy(t), nc.Probe(t)
        if which == "dup_second":     # (a) a duplicated address with the second slot's MAC
            k = an["dup"][0]
            s = [s for s in range(p.cap) if p.valid[s] and p.keys[s] == k and
                 s != an["reachable"][k]][0]
        elif which == "hidden":       # (b) a hidden entry's address and MAC
            k = an["hidden"][0]
            s = [s for s in range(p.cap) if p.valid[s] and p.keys[s] == k][0]
        elif which == "zero_arp":     # (c) last_arp_ip = 0 with a MAC the table does not give
            if fam == "ndp":
                continue
            assert 0 in an["reachable"]
            l1[macf] = np.frombuffer(bytes.fromhex("02c0ffee0001"), np.uint8)
            continue
        else:                         # (d) the calloc'd state, the table holding ::
            assert fam == "arp" or bytes(16) in an["reachable"]
            continue
        l1[ipf] = k if fam == "arp" else np.frombuffer(k, np.uint8)
        l1[macf] = np.frombuffer(p.macs[s], np.uint8)
    return l1


_L1_WL: dict = {}


def l1_workload(name, which):
    """(workload, starting L1) of an interplay test: the case's batch with the first 40 packets of
    each family sent to the address the starting entry names (a whole wave of L1 hits before the
    first table hit), for (c) and (d) to 0.0.0.0 and ::."""
    from test_gpu_parity import _force_dst

    if (name, which) not in _L1_WL:
        wl = workload(name).copy()
        l1 = l1_start(which, nc.case(name))
        _force_dst(wl, 40, int(l1["last_arp_ip"][0]), l1["last_ndp_ip"][0])
        _L1_WL[name, which] = (wl, l1)
    return _L1_WL[name, which]


@pytest.mark.parametrize("which", L1_STARTS)
@pytest.mark.parametrize("name", ["combo", "embed:combo"])
def test_l1_starts_take_effect(name, which):
    """Each starting state names what it should, and the oracle's first batch shows it: packets to
    the named address carry the L1 entry's MAC, not the table's, until a table hit replaces it."""
    wl, l1 = l1_workload(name, which)
    r = oracle.run_restated(wl, l1=l1)
    check_against_reference(wl, r, f"{name} {which}", l1=l1)
    model = check_model(wl, r, f"{name} {which}", l1=l1)
    fams, dsts = nc.destinations(wl)
    offs = desc_offsets(wl.desc)
    if which in ("dup_second", "hidden"):
        for f, ip, mac in ((4, int(l1["last_arp_ip"][0]), l1["last_arp_mac"][0].tobytes()),
                           (6, l1["last_ndp_ip"][0].tobytes(), l1["last_ndp_mac"][0].tobytes())):
            got = [i for i, m in enumerate(model) if m is not None and fams[i] == f and
                   dsts[i] == ip and m[2] == "l1" and m[1] == mac]
            assert len(got) > 20, f"family {f}: {len(got)} packets took the starting entry's MAC"
            assert nc.Probe(wl.arp if f == 4 else wl.ndp).mac(ip) != mac
            o = int(offs[got[0]])
            assert r.frames[o:o + 6].tobytes() == mac
    if which == "zero_arp":
        # the reference never consults an entry for 0.0.0.0: its MAC reaches no frame
        mac = l1["last_arp_mac"][0].tobytes()
        assert all(m[1] != mac for m in model if m is not None and m[0])
        to0 = [i for i, m in enumerate(model) if m is not None and fams[i] == 4 and dsts[i] == 0]
        assert len(to0) > 30 and all(model[i][2] == "table" for i in to0)
    if which == "calloc_zero6":
        first = [i for i in range(wl.n) if fams[i] == 6][:40]
        took = [i for i in first if model[i] is not None]
        assert len(took) > 20 and all(model[i] == (True, bytes(6), "l1") for i in took)
