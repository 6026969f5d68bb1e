"""Adversarial rule tables through every device matcher, against the oracle bit for bit.

The tables of tests/test_rule_index.py (version-0 rules, masks that are not prefixes, IPv4 views
of IPv6 masks, no catch-all, few values with many overlaps) and tables that sit on the sizes the
rule compiler branches on (upe_rules.cpp build_image: `pad > kSmallRules` turns at 61 rules, the
sorted index rides in x1 below 8192 rules, fam_all 1 / 2 / 3, an empty family list, a tuple-space
group too large to stage), with traffic cut from the rules' own edges (boundary_keys, one-bit
flips inside and outside a rule's mask, keys of the other family) and made into frames
(keyframes.frames_from_keys).  Each table runs under the compiler's own choice and with the LDS /
family-list / whole-table scan, the decision tree (staged or read from memory) and the
tuple-space index (fingerprints staged or not) forced; verdict words, frames, counters,
rule_stats and L1 must equal the C restatement's (and, where the reference worker is built, the
restatement must equal the worker).

The CPU tests pin the generators: the frames parse back to their keys, and the oracle's verdicts
show that every table's traffic reaches matches, misses, deep rules and all four outcomes, so the
GPU comparison cannot pass on a degenerate batch.
"""
from __future__ import annotations

import numpy as np
import pytest

import oracle
from keyframes import arrange_runs, canonical, frames_from_keys, run_kinds
from test_gpu_parity import _assert_same, _run
from test_rule_index import boundary_keys, random_table
from upe_amd import gpu, layout, synth
from upe_amd.layout import (ACT_DROP, ACT_FWD, FLOW_KEY_DTYPE, RULE_DTYPE, V_DROP_NOMATCH,
                            V_DROP_RULE, V_FWD, VF_NEIGH_HIT)

N_PACKETS = 4096 + 37   # a ragged last chunk
SMALL = 61              # build_image: pad = (ceil(count / 4) + 1) * 4 > kSmallRules (64)

_MATCH = ("src_ip", "src_mask", "dst_ip", "dst_mask", "src_port", "dst_port", "protocol",
          "ip_ver")


# ---------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------

def _family_only(rng, n, ver):
    r = random_table(rng, n, True)
    r["ip_ver"] = ver
    return r


def _deep_table(rng, n):
    """random_table(prefix_masks=True) with its broad rules moved last: a rule that constrains
    fewer than two of its five fields gets a priority past every other rule's (random_table
    draws priorities below 2^20).  Among thousands of rules over few values, the broad ones
    otherwise take every key within the first few hundred entries, and nothing deep is reached."""
    r = random_table(rng, n, True)
    fields = (r["src_mask"].any(axis=1).astype(int) + r["dst_mask"].any(axis=1) +
              (r["src_port"] != 0) + (r["dst_port"] != 0) + (r["protocol"] != 0))
    r["priority"] = np.where(fields < 2, r["priority"] | np.uint32(1 << 21), r["priority"])
    return r


def _catchall_first(rng, fams):
    """A rule matching every key of each family in `fams` at priority 0, then ~100 rules of the
    other family (or of both).  The IPv4 catch-all forwards, the IPv6 one drops (both_*) or
    forwards (v6_*), so that the batch still holds every outcome."""
    body = random_table(rng, 100, True)
    if fams != (4, 6):
        body["ip_ver"] = 6 if fams == (4,) else 4
    head = [synth.make_rule(0, ACT_FWD if f == 4 or fams == (6,) else ACT_DROP, ip_ver=f)
            for f in fams]
    return np.concatenate([synth.rules_array(head), body])


def _dups_ties(rng):
    """40 distinct rules, five copies each, the copies' actions alternating; the copies of half
    of the rules share one priority (rule_id breaks the tie), the others' differ.  Inserted in a
    shuffled order."""
    base = random_table(rng, 40, True)
    r = np.repeat(base, 5)
    copy = np.tile(np.arange(5), 40)
    tie = np.repeat(rng.random(40) < 0.5, 5)
    r["action"] = (r["action"] + copy) % 2
    r["priority"] = np.where(tie, r["priority"], r["priority"] + rng.permutation(200) % 7)
    return r[rng.permutation(200)]


_BASE = None


def _base():
    """The rest of the workload: config C's ARP and NDP tables, port identity and L1 state."""
    global _BASE
    if _BASE is None:
        _BASE = synth.config_c(n=64, seed=3)
    return _BASE


def _tss_big_group(rng):
    """~5000 exact IPv4 and ~3000 exact IPv6 5-tuples (one signature per family, each group past
    kFpStageGroup slots: never staged), 200 rules in 10 small prefix signatures (6 IPv4, 4 IPv6:
    staged, and ng4 != ng6) cut from the exact rules' own addresses, and a final catch-all.  Half
    of the exact rules' destinations are addresses the neighbour tables hold."""
    base = _base()
    arp_ip = base.arp["ip"][base.arp["valid"] == 1]
    ndp_ip = base.ndp["ip"][base.ndp["valid"] == 1]
    n4, n6, nsig, per = 5000, 3000, 10, 20
    n = n4 + n6 + nsig * per + 1
    r = np.zeros(n, RULE_DTYPE)
    r["priority"][:n - 1] = rng.permutation(n - 1) + 1
    r["action"] = rng.integers(0, 2, size=n)
    r["out_ifindex"] = r["action"]
    # exact flows
    r["ip_ver"][:n4] = 4
    r["ip_ver"][n4:n4 + n6] = 6
    ex = n4 + n6
    r["protocol"][:ex] = rng.choice([1, 6, 17], size=ex)
    r["src_port"][:ex] = rng.integers(1, 65536, size=ex)
    r["dst_port"][:ex] = rng.integers(1, 65536, size=ex)
    src4 = (0x0B000000 + rng.integers(0, 1 << 24, size=n4)).astype("<u4")
    dst4 = np.where(rng.random(n4) < 0.5, arp_ip[rng.integers(0, len(arp_ip), size=n4)],
                    0xAC100000 + rng.integers(0, 1 << 20, size=n4)).astype("<u4")
    r["src_ip"][:n4, :4] = src4.view(np.uint8).reshape(-1, 4)
    r["dst_ip"][:n4, :4] = dst4.view(np.uint8).reshape(-1, 4)
    r["src_mask"][:n4, :4] = 0xFF
    r["dst_mask"][:n4, :4] = 0xFF
    src6 = rng.integers(0, 256, size=(n6, 16), dtype=np.uint8)
    src6[:, :4] = np.frombuffer(synth.V6_SRC_PRE, np.uint8)
    dst6 = rng.integers(0, 256, size=(n6, 16), dtype=np.uint8)
    dst6[:, :4] = np.frombuffer(synth.V6_DST_PRE, np.uint8)
    held = rng.random(n6) < 0.5
    dst6[held] = ndp_ip[rng.integers(0, len(ndp_ip), size=int(held.sum()))]
    r["src_ip"][n4:ex] = src6
    r["dst_ip"][n4:ex] = dst6
    r["src_mask"][n4:ex] = 0xFF
    r["dst_mask"][n4:ex] = 0xFF
    # prefix signatures: (family, source prefix, destination prefix, protocol?, dst port?)
    sigs = [(4, 24, 0, False, False), (4, 16, 32, False, False), (4, 0, 24, True, False),
            (4, 28, 0, False, True), (4, 20, 20, True, True), (4, 12, 0, True, False),
            (6, 64, 0, False, False), (6, 96, 128, False, False), (6, 0, 120, True, False),
            (6, 48, 0, False, True)]
    for s, (fam, ls, ld, hp, hd) in enumerate(sigs):
        for i in range(ex + s * per, ex + (s + 1) * per):
            j = int(rng.integers(0, n4)) if fam == 4 else n4 + int(rng.integers(0, n6))
            r[i]["ip_ver"] = fam
            for a, m, ln in (("src_ip", "src_mask", ls), ("dst_ip", "dst_mask", ld)):
                if ln == 0:
                    continue
                if fam == 4:
                    mk = np.zeros(16, np.uint8)
                    mk[:4] = np.frombuffer(np.uint32(synth.ipv4_mask(ln)).astype("<u4").tobytes(),
                                           np.uint8)
                else:
                    mk = np.frombuffer(synth.ipv6_mask(ln), np.uint8)
                r[i][m] = mk
                r[i][a] = r[j][a] & mk
            if hp:
                r[i]["protocol"] = r[j]["protocol"]
            if hd:
                r[i]["dst_port"] = r[j]["dst_port"]
    r[n - 1] = synth.make_rule(1 << 30, ACT_DROP)
    return r


TABLES = {
    "rand_prefix_60": (160, lambda g: random_table(g, 60, True)),
    "rand_prefix_61": (161, lambda g: random_table(g, 61, True)),
    "rand_prefix_64": (165, lambda g: random_table(g, 64, True)),
    "rand_prefix_65": (165, lambda g: random_table(g, 65, True)),
    "rand_prefix_300": (104, lambda g: random_table(g, 300, True)),
    "rand_bits_61": (261, lambda g: random_table(g, 61, False)),
    "rand_bits_300": (115, lambda g: random_table(g, 300, False)),
    "only_v6_100": (320, lambda g: _family_only(g, 100, 6)),
    "only_v4_100": (320, lambda g: _family_only(g, 100, 4)),
    "v4_catchall_first": (404, lambda g: _catchall_first(g, (4,))),
    "v6_catchall_first": (411, lambda g: _catchall_first(g, (6,))),
    "both_catchall_first": (410, lambda g: _catchall_first(g, (4, 6))),
    "dups_ties_200": (500, _dups_ties),
    "idx_8191": (8191, lambda g: _deep_table(g, 8191)),
    "idx_8192": (8192, lambda g: _deep_table(g, 8192)),
    "tss_big_group": (700, _tss_big_group),
}
CATCHALL_FIRST = ("v4_catchall_first", "v6_catchall_first", "both_catchall_first")
BIG = ("idx_8191", "idx_8192", "tss_big_group")
ALL_MODES = ("default", "scan", "tree", "tree-memory", "tss", "tss-unstaged")
CASES = [(t, m) for t in TABLES for m in ALL_MODES
         if t not in BIG or m in ("default", "scan", "tree") or
         (t == "tss_big_group" and m == "tss-unstaged")]


# ---------------------------------------------------------------------------------------------
# traffic
# ---------------------------------------------------------------------------------------------

def own_keys(rs, rng, n, flip=False):
    """Keys that match the rule they are cut from (the rule's value, its free bits random) and,
    with `flip`, the same with exactly one bit of one address word flipped: inside the rule's
    mask for every other key (a near miss of that rule), outside it for the rest (still a match),
    or the other way where the mask leaves no such bit."""
    keys = np.zeros(n, FLOW_KEY_DTYPE)
    for i, j in enumerate(rng.integers(0, len(rs), size=n)):
        r = rs[j]
        ver = int(r["ip_ver"]) or int(rng.choice([4, 6]))
        keys[i]["ip_ver"] = ver
        for a, m in (("src_ip", "src_mask"), ("dst_ip", "dst_mask")):
            mk = r[m].astype(np.uint8)
            keys[i][a] = (r[a] & mk) | (rng.integers(0, 256, 16, dtype=np.uint8) & ~mk)
        keys[i]["src_port"] = int(r["src_port"]) or int(rng.integers(0, 65536))
        keys[i]["dst_port"] = int(r["dst_port"]) or int(rng.integers(0, 65536))
        keys[i]["protocol"] = int(r["protocol"]) or int(rng.choice([1, 6, 17]))
        if flip:
            a, m = (("src_ip", "src_mask"), ("dst_ip", "dst_mask"))[int(rng.integers(0, 2))]
            bits = np.unpackbits(r[m].astype(np.uint8)[:4 if ver == 4 else 16])
            cand = np.nonzero(bits == (1 - i % 2))[0]
            if cand.size == 0:
                cand = np.arange(bits.size)
            b = int(rng.choice(cand))
            k = keys[i][a].copy()
            k[b // 8] ^= 0x80 >> (b % 8)
            keys[i][a] = k
    return keys


def traffic(name, rs, rng, base):
    n = N_PACKETS
    if name == "tss_big_group":
        # the rules' own tuples (a hit in either cuckoo slot) and one-bit near misses; the
        # destinations come from the rules, half of which name a neighbour the tables hold
        keys = np.concatenate([own_keys(rs, rng, n // 2), own_keys(rs, rng, n - n // 2, flip=True)])
        return arrange_runs(canonical(keys)[rng.permutation(n)])
    nb = n * 3 // 5
    keys = np.concatenate([boundary_keys(rs, rng, nb), own_keys(rs, rng, n - nb, flip=True)])
    keys = keys[rng.permutation(n)]
    # an eighth of the keys in the other family: a rule's bytes under the other view, and the
    # only traffic an empty family list ever sees
    other = rng.random(n) < 0.125
    keys["ip_ver"] = np.where(other, 10 - keys["ip_ver"], keys["ip_ver"])
    # a third of the destinations are neighbours the tables hold: forwarded packets then take
    # the found branch as well as the not-found one
    arp_ip = base.arp["ip"][base.arp["valid"] == 1].astype("<u4")
    ndp_ip = base.ndp["ip"][base.ndp["valid"] == 1]
    for i in np.nonzero(rng.random(n) < 1 / 3)[0]:
        if keys[i]["ip_ver"] == 4:
            d = np.zeros(16, np.uint8)
            d[:4] = np.frombuffer(arp_ip[rng.integers(0, len(arp_ip))].tobytes(), np.uint8)
        else:
            d = ndp_ip[rng.integers(0, len(ndp_ip))]
        keys[i]["dst_ip"] = d
    return arrange_runs(canonical(keys))


_WL: dict = {}
_ORACLE: dict = {}


def workload(name):
    if name not in _WL:
        seed, make = TABLES[name]
        rng = np.random.default_rng(seed)
        base = _base()
        rules = synth.build_rule_table(make(rng))
        keys = traffic(name, rules, rng, base)
        frames, desc = frames_from_keys(keys, rng)
        cap = 1024
        while cap < len(rules):
            cap *= 2
        wl = synth.Workload(name, frames, desc, rules, cap, base.arp.copy(), base.ndp.copy(),
                            base.eth_addr, base.ip4_addr, base.l1.copy())
        _WL[name] = (wl, keys)
    return _WL[name]


def oracle_of(name):
    """One restated run per table (the idx_* scans are the slowest CPU part), pinned to the
    reference worker itself where it is built."""
    if name not in _ORACLE:
        wl, _ = workload(name)
        r = oracle.run_restated(wl)
        if oracle.ref_available():
            ref = oracle.run_reference(wl)
            assert np.array_equal(ref.verdict, r.verdict), f"{name}: restatement vs worker"
            assert np.array_equal(ref.frames, r.frames)
            assert ref.counters.tobytes() == r.counters.tobytes()
            assert np.array_equal(ref.rule_stats, r.rule_stats)
            assert ref.l1.tobytes() == r.l1.tobytes()
        _ORACLE[name] = r
    return _ORACLE[name]


def _first_catchall(rs):
    """Per family, the sorted index of the first rule that matches every key of it (or None)."""
    wild = ~(rs["src_mask"].any(axis=1) | rs["dst_mask"].any(axis=1) | (rs["src_port"] != 0) |
             (rs["dst_port"] != 0) | (rs["protocol"] != 0))
    # (an IPv4 key tests only bytes 0-3 of a mask)
    wild4 = ~(rs["src_mask"][:, :4].any(axis=1) | rs["dst_mask"][:, :4].any(axis=1) |
              (rs["src_port"] != 0) | (rs["dst_port"] != 0) | (rs["protocol"] != 0))
    out = {}
    for fam, w in ((4, wild4), (6, wild)):
        idx = np.nonzero(w & ((rs["ip_ver"] == 0) | (rs["ip_ver"] == fam)))[0]
        out[fam] = int(idx[0]) if idx.size else None
    return out


# ---------------------------------------------------------------------------------------------
# CPU: the generators
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prefix_masks", [True, False])
def test_frames_parse_back_to_their_keys(prefix_masks):
    """boundary_keys output (every protocol, both families, bytes past an IPv4 address) through
    frames_from_keys: the oracle's parser returns rc 0 and the identical key for every frame."""
    rng = np.random.default_rng(21)
    rs = random_table(rng, 120, prefix_masks)
    keys = arrange_runs(boundary_keys(rs, rng, 1500))
    frames, desc = frames_from_keys(keys, rng)
    want = canonical(keys)
    offs, lens = layout.desc_offsets(desc), layout.desc_lens(desc)
    assert lens.min() >= 64 and lens.max() <= 200 and len(np.unique(lens)) > 50
    assert run_kinds(keys) == {"v4", "v6", "mixed"}
    seen = set()
    for i in range(len(keys)):
        o, ln = int(offs[i]), int(lens[i])
        rc, k = oracle.parse(bytes(frames[o:o + ln]), ln)
        assert rc == 0, f"frame {i} does not parse"
        assert k.tobytes() == want[i:i + 1].tobytes(), f"frame {i}: {k} vs {want[i]}"
        seen.add((int(want[i]["ip_ver"]), int(want[i]["protocol"])))
        if want[i]["ip_ver"] == 4:
            assert frames[o + 22] >= 2
            seen.add(("ihl", int(frames[o + 14] & 0xF) > 5))
        else:
            assert frames[o + 21] >= 2
    assert seen >= {(v, p) for v in (4, 6) for p in (1, 6, 17)} | {("ihl", True), ("ihl", False)}


@pytest.mark.parametrize("name", list(TABLES))
def test_traffic_is_not_hollow(name):
    """On the oracle's verdicts alone: the batch matches and misses, reaches the end of the
    table, takes every outcome, and holds all-IPv4, all-IPv6 and mixed 64-packet runs."""
    wl, keys = workload(name)
    rs = wl.rules_sorted
    r = oracle_of(name)
    n = wl.n
    assert n == N_PACKETS and run_kinds(keys) == {"v4", "v6", "mixed"}
    code = r.verdict & 0xF
    idx = (r.verdict >> 8).astype(np.int64) - 1
    assert (code != 0).all(), "a frame did not parse"
    matched = idx >= 0
    first = _first_catchall(rs)
    any_catchall = first[4] is not None or first[6] is not None
    if name not in CATCHALL_FIRST:
        assert matched.mean() >= 0.20, f"{matched.mean():.3f} matched"
    if not any_catchall:
        assert (~matched).mean() >= 0.05, f"{(~matched).mean():.3f} unmatched"
    if name != "both_catchall_first":
        # (both_catchall_first: every key stops at sorted index 0 or 1, by construction)
        assert idx.max() >= len(rs) * 3 // 4, f"deepest match {idx.max()} of {len(rs)}"
    found = (code == V_FWD) & ((r.verdict & VF_NEIGH_HIT) != 0)
    lost = (code == V_FWD) & ((r.verdict & VF_NEIGH_HIT) == 0)
    classes = {"fwd_found": found.mean(), "fwd_not_found": lost.mean(),
               "drop_rule": (code == V_DROP_RULE).mean()}
    if first[4] is None or first[6] is None:   # a key of some family can go unmatched
        classes["no_match"] = (code == V_DROP_NOMATCH).mean()
    assert min(classes.values()) >= 0.02, classes
    if name == "dups_ties_200":
        same = [b"".join(np.asarray(rs[i][f]).tobytes() for f in _MATCH) for i in range(len(rs))]
        later = np.array([same[i] in same[i + 1:] for i in range(len(rs))])
        assert later[idx[matched]].mean() >= 0.10
        # both kinds of copy: ties broken by rule_id, and distinct priorities
        p = rs["priority"]
        assert (p[1:] == p[:-1]).sum() > 20 and len(np.unique(p)) > 60
    if name == "idx_8192":
        assert idx.max() >= 4096   # bit 12 of the index carried in x1
    if name == "only_v4_100":
        assert (rs["ip_ver"] == 4).all() and (keys["ip_ver"] == 6).mean() > 0.05
    if name == "only_v6_100":
        assert (rs["ip_ver"] == 6).all() and (keys["ip_ver"] == 4).mean() > 0.05


def test_tables_sit_on_the_compiler_thresholds():
    """The shapes the table ids promise, from the sorted tables alone."""
    n = {t: len(workload(t)[0].rules_sorted) for t in TABLES}
    assert [n[f"rand_prefix_{k}"] for k in (60, 61, 64, 65, 300)] == [60, 61, 64, 65, 300]
    assert n["idx_8191"] == 8191 and n["idx_8192"] == 8192
    for t, want in (("v4_catchall_first", {4: 0}), ("v6_catchall_first", {6: 0}),
                    ("both_catchall_first", {4: 0, 6: 1})):
        first = _first_catchall(workload(t)[0].rules_sorted)
        assert {f: first[f] for f in want} == want, (t, first)
        assert n[t] >= SMALL
    rs = workload("tss_big_group")[0].rules_sorted
    exact = rs["src_mask"].all(axis=1) & rs["dst_mask"].all(axis=1)
    exact4 = (rs["ip_ver"] == 4) & rs["src_mask"][:, :4].all(axis=1) & \
        rs["dst_mask"][:, :4].all(axis=1) & (rs["src_port"] != 0)
    # a group of g keys takes the power of two >= 2.5 g slots (kTssRatioX2): past kFpStageGroup
    assert (exact & (rs["ip_ver"] == 6)).sum() * 5 // 2 > 4096 and exact4.sum() * 5 // 2 > 4096


# ---------------------------------------------------------------------------------------------
# GPU: every matcher on every table
# ---------------------------------------------------------------------------------------------

def _set_mode(monkeypatch, mode):
    if mode == "default":
        for k in ("UPE_GPU_TSS", "UPE_GPU_TREE", "UPE_GPU_TREE_LDS", "UPE_GPU_FP_STAGE"):
            monkeypatch.delenv(k, raising=False)
        return
    monkeypatch.setenv("UPE_GPU_TSS", "1" if mode.startswith("tss") else "0")
    monkeypatch.setenv("UPE_GPU_TREE", "0" if mode == "scan" else "1")
    monkeypatch.setenv("UPE_GPU_TREE_LDS", "0" if mode == "tree-memory" else "1")
    monkeypatch.setenv("UPE_GPU_FP_STAGE", "0" if mode.endswith("unstaged") else "1")


def _recording(factory, seen):
    """The worker factory, with the index kind, the tree's node count and the last launch's
    variant noted as a worker closes (test_gpu_parity._run owns the worker)."""
    def make(capacity):
        w = factory(capacity)
        close = w.close

        def closing():
            if w._ctx:
                seen.update(kind=w.rule_index_kind(), nodes=int(w.rule_index_info()["nodes"]),
                            variant=int(w.launch_info()["variant"]))
            close()
        w.close = closing
        return w
    return make


def _check(gpu_worker_factory, monkeypatch, name, mode, emit):
    _set_mode(monkeypatch, mode)
    wl, _ = workload(name)
    r = oracle_of(name)
    nrules = len(wl.rules_sorted)
    seen = {}
    frames, verdict, counters, stats, l1 = _run(_recording(gpu_worker_factory, seen), wl, emit=emit)
    kind, nodes, variant = seen["kind"], seen["nodes"], seen["variant"]
    scan = variant & gpu.VAR_SCAN
    what = f"{name} {mode} emit={emit}: {nrules} rules, kind {kind}, variant {variant:#x}"
    print(what)
    if mode.startswith("tss"):
        assert kind == 1, what
    elif mode == "scan":
        assert kind == 0, what
        if nrules >= SMALL:
            assert scan in (gpu.VAR_FAM, gpu.VAR_GLB), what
        else:
            assert scan == 0, what
        if name in CATCHALL_FIRST:
            assert scan == gpu.VAR_GLB, what
        if name in ("only_v4_100", "only_v6_100"):
            assert scan == gpu.VAR_FAM, what
    elif mode.startswith("tree"):
        if nrules >= SMALL:   # pad > kSmallRules: 61 rules, not 65
            assert nodes > 0, what + ": the table got no tree"
            assert kind == 2 and scan == gpu.VAR_TREE, what
        else:
            assert kind == 0 and scan == 0, what
    elif name == "tss_big_group":
        assert kind == 1, what
    _assert_same((frames, verdict, counters, stats, l1),
                 {"verdict": r.verdict, "frames": r.frames, "counters": r.counters,
                  "rule_stats": r.rule_stats, "l1": r.l1}, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", CASES)
def test_adversarial_table(gpu_worker_factory, monkeypatch, name, mode):
    _check(gpu_worker_factory, monkeypatch, name, mode, emit=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TABLES))
def test_adversarial_table_emit(gpu_worker_factory, monkeypatch, name):
    """The compiler's own choice of index in emit mode (records applied to the frames)."""
    _check(gpu_worker_factory, monkeypatch, name, "default", emit=True)
