"""CPU: the tables and batches of tests/accounting_cases.py have the answers they claim.

For every table size, one packet per targeted rule (every rule, or for the largest tables a stride
that keeps every boundary index) and every batch shape at a few small sizes run through the C
restatement (and the reference worker, where it is built; its 2048-byte pktbufs get the long frames
cut to that): the verdicts' codes and rule bits, the
rule_stats and the counters must equal what the generator computes as a bincount.  The restatement
scans the table linearly, which bounds the packets for the 64k-rule tables.  After this,
tests/test_gpu_accounting.py trusts the bincount at sizes no CPU test runs in seconds.  The named
batches must also reach what they are named for: the sizes on either side of the group-by's
vector / tail split, the boundary indexes of its ranges and of the 4-byte key.
"""
from __future__ import annotations

import numpy as np
import pytest

import accounting_cases as ac
import oracle
from upe_amd.layout import PKTBUF_DATA

MOST = ac.MOST                    # targeted rules of a table past this size
CPU_SIZES = (1, 63, 64, 65, 2048)
REF_MOST = PKTBUF_DATA          # the longest frame the reference worker takes
REF_RULES = 1000                  # the reference worker sorts on every insert: tables up to here
BIG_SIZES = (65, 2048)            # the restatement scans linearly: the 16k+ tables' batches
CODE_AND_RULE = np.uint32(0xFFFFFF0F)   # a verdict word without its flags


def check(t, batches, what):
    """Each batch through the oracle from the state the one before left; everything equals the
    generator's claim."""
    cnt = st = None
    for k, b in enumerate(batches):
        wl = ac.workload(t, b)
        r = oracle.run_restated(wl, rules_sorted=t.rules_sorted, counters=cnt, rule_stats=st)
        cnt, st = r.counters, r.rule_stats
        want_c, want_s = ac.expected(t, batches[:k + 1])
        tag = f"{what} {b.name}"
        assert np.array_equal(r.verdict & CODE_AND_RULE, ac.expected_verdict(t, b)), tag
        assert np.array_equal(st, want_s), tag
        assert cnt.tobytes() == want_c.tobytes(), (tag, cnt, want_c)
        if oracle.ref_available() and t.nrules <= REF_RULES:
            # the worker's pktbuf holds 2048 bytes: it gets the same batch with the 65535-byte
            # frames cut to that, from the same builder
            twin = b if b.lens.max() <= REF_MOST else ac.build(t, b.name, b.target,
                                                               np.minimum(b.lens, REF_MOST))
            ref = oracle.run_reference(ac.workload(t, twin))
            one_c, one_s = ac.expected(t, [twin])
            assert np.array_equal(ref.rules_sorted, t.rules_sorted), tag
            assert np.array_equal(ref.verdict, r.verdict), tag
            assert np.array_equal(ref.rule_stats, one_s), tag
            assert ref.counters.tobytes() == one_c.tobytes(), tag


def test_sizes_come_from_the_constants():
    assert ac.nrules_pad(ac.SMALL_LAST) == ac.K_SMALL_RULES < ac.nrules_pad(ac.SMALL_LAST + 1)
    assert ac.nrules_pad(ac.LDS_LAST) == ac.K_LDS_STATS_MAX < ac.nrules_pad(ac.LDS_LAST + 1)
    want = {8: "small", ac.SMALL_LAST: "small", ac.SMALL_LAST + 1: "mid", 1000: "mid",
            ac.LDS_LAST: "mid", ac.LDS_LAST + 1: "group-by", ac.K_HIST_RANGE: "group-by",
            ac.K_HIST_RANGE + 1: "group-by", ac.K_GB_PACKED: "group-by",
            ac.K_GB_PACKED + 1: "group-by"}
    assert {n: ac.stats_path(n) for n in ac.TABLE_SIZES} == want
    assert len(set(ac.TABLE_SIZES)) == 10
    # the group-by's vector rounds take 16 packets a thread: the sizes straddle a multiple of 16
    tail = [n for n in ac.BATCH_SIZES if n % 16]
    assert ac.K_HIST_CHUNK_MIN % 16 == 0 and ac.K_HIST_CHUNK_MIN in ac.BATCH_SIZES
    assert {ac.K_HIST_CHUNK_MIN - 1, ac.K_HIST_CHUNK_MIN + 1, ac.K_HIST_CHUNK_MIN + 15,
            2 * ac.K_HIST_CHUNK_MIN + 1, 40005} <= set(tail)
    assert 2 * ac.K_HIST_CHUNK_MIN + 1 > 2 * ac.K_HIST_CHUNK_MIN   # a third chunk of one packet
    assert ac.K_WG_PACKETS * 65535 < 1 << 32 <= (ac.K_WG_PACKETS + 2) * 65535


@pytest.mark.parametrize("nrules", ac.TABLE_SIZES)
def test_table(nrules):
    t = ac.table(nrules)
    rs = t.rules_sorted
    assert len(rs) == nrules and np.array_equal(rs["priority"], np.arange(nrules))
    assert np.array_equal(rs["rule_id"], t.rule_id)
    assert np.array_equal(t.sorted_index[t.rule_id], np.arange(nrules))
    if nrules > 8:
        assert not np.array_equal(t.rule_id, np.arange(nrules)), "rule_id and sorted index coincide"
    pairs = rs["src_port"].astype(np.int64) << 16 | rs["dst_port"]
    assert len(np.unique(pairs)) == nrules and (rs["src_port"] > 0).all() and (rs["dst_port"] > 0).all()
    assert (rs["src_port"] < ac.NOMATCH_PORTS[0]).all()
    assert abs(int(t.drops.sum()) - nrules / 2) <= 1 and t.capacity >= nrules
    b = t.boundaries()
    assert b["first"] == 0 and b["last"] == nrules - 1
    assert ("range1_first" in b) == (nrules > ac.K_HIST_RANGE)
    assert ("key_max" in b) == (nrules >= ac.K_GB_PACKED)
    assert ("past_key" in b) == (nrules > ac.K_GB_PACKED)
    sample = ac.sample_rules(t, MOST)
    assert set(b.values()) <= set(sample.tolist()) and len(sample) <= MOST + 32
    assert t.drops[sample].any() and not t.drops[sample].all()
    if nrules <= MOST:
        assert len(sample) == nrules


@pytest.mark.parametrize("nrules", ac.TABLE_SIZES)
def test_one_packet_per_rule(nrules):
    t = ac.table(nrules)
    rules = ac.sample_rules(t, MOST)
    target = np.concatenate([rules, [ac.NONE]])
    b = ac.build(t, "each-once", target, ac.rule_len(t, np.maximum(target, 0), ac._long_set(t, rules)))
    assert set(ac.LENS) <= set(b.lens.tolist())
    check(t, [b], f"{nrules} rules")


@pytest.mark.parametrize("nrules", ac.TABLE_SIZES)
def test_batch_shapes(nrules):
    t = ac.table(nrules)
    for n in CPU_SIZES if nrules <= REF_RULES else BIG_SIZES:
        batches = ac.shapes(t, n, MOST)
        names = [b.name.split(":")[0] for b in batches]
        assert names.count("one") == len(t.boundaries()) and names[-3:] == ["every", "nothing",
                                                                            "interleaved"]
        check(t, batches, f"{nrules} rules")


@pytest.mark.parametrize("nrules", ac.TABLE_SIZES)
def test_batches_reach_what_they_are_named_for(nrules):
    t = ac.table(nrules)
    bnd = t.boundaries()
    for n in ac.BATCH_SIZES:
        batches = ac.shapes(t, n)        # as tests/test_gpu_accounting.py builds them
        for (which, idx), b in zip(bnd.items(), batches):
            assert b.n == n and (b.target == idx).all(), b.name
            if t.drops[idx] and n >= 3:
                assert set(b.lens.tolist()) == set(ac.LENS) and b.shared == n - 3, b.name
            else:
                assert b.shared == 0 and b.lens.max() <= 200, b.name
        every, none, mixed = batches[-3:]
        assert (none.target == ac.NONE).all() and none.n == n
        for b in (every, mixed):
            hit = b.target >= 0
            assert b.n == n and t.drops[b.target[hit]][b.lens[hit] > 200].all(), b.name
            if n >= 64:   # the boundary rules lead the order
                assert set(bnd.values()) <= set(b.target.tolist()), b.name
                assert (b.lens == ac.LENS[2]).any() and (b.lens == ac.LENS[1]).any()
        assert ac.groups_mixed(mixed) and (n < 3 or (mixed.target == ac.NONE).any())
        if n >= ac.K_HIST_CHUNK_MIN - 1:
            _reaches_every_range(t, n, every, mixed)


def _reaches_every_range(t, n, every, mixed):
    """From the first size past a chunk on, `every` and `interleaved` hit every rule they aim at:
    the whole table where the batch has room for it, else a stride whose gaps stay far below a
    range, so every group-by range is hit in its interior (not only at its boundary indexes, nor
    only in the table's lowest indexes), every rule with its own length, and in `every` with
    counts that differ inside every range."""
    aimed = ac.sample_rules(t, ac.most_for(t, n))
    if 4 * t.nrules <= n:
        assert np.array_equal(aimed, np.arange(t.nrules))
    near = {v + d for v in t.boundaries().values() for d in (-1, 0, 1)}
    for b in (every, mixed):
        hit_rules, counts = np.unique(b.target[b.target >= 0], return_counts=True)
        assert np.array_equal(hit_rules, aimed), b.name
        lens_of = np.zeros(t.nrules, np.int64)
        lens_of[b.target[b.target >= 0]] = b.lens[b.target >= 0]
        assert np.array_equal(lens_of[b.target[b.target >= 0]], b.lens[b.target >= 0]), b.name
        for r0, r1 in ac.ranges(t):
            inside = (hit_rules >= r0) & (hit_rules < r1)
            interior = [int(r) for r in hit_rules[inside] if int(r) not in near]
            room = r1 - r0 - sum(r0 <= v < r1 for v in near)
            # a range one rule wide is its boundary index; a whole one has hundreds of interior
            # hits, no two further apart than a hundredth of it
            if room > 0:
                assert len(interior) >= min(room, ac.K_HIST_RANGE // 64), (b.name, r0)
                gaps = np.diff(np.concatenate([[r0 - 1], hit_rules[inside], [r1]]))
                assert gaps.max() <= max(1, ac.K_HIST_RANGE // 100), (b.name, r0, int(gaps.max()))
                # (the 8-rule table's dropping rules all carry the longest frames)
                assert len(set(lens_of[interior].tolist())) >= min(7, len(interior) // 2), (b.name, r0)
            assert inside.any(), (b.name, r0)
            if b is every:
                assert len(np.unique(counts[inside])) >= min(7, int(inside.sum())), (b.name, r0)


def test_byte_bin_batch():
    """The batch that cannot fit 32-bit bins on eight workgroups, checked in its first packets
    against the oracle (the rest are the same 64 frames again)."""
    for nrules in (8, 1000):
        t = ac.table(nrules)
        b = ac.byte_bin_batch(t)
        idx = int(b.target[0])
        assert t.drops[idx] and b.n == 1 << 20 and (b.lens == 65535).all()
        assert b.n * 65535 > 8 << 32
        offs = (b.desc >> np.uint64(16)).astype(np.int64)
        assert len(np.unique(offs)) == ac.BYTE_BIN_FRAMES
        assert offs.max() + 65535 + 96 <= len(b.frames), "a descriptor leaves its allocation"
        head = ac.Batch("byte-bin-head", b.target[:256], b.lens[:256], b.frames, b.desc[:256], 192)
        check(t, [head], f"{nrules} rules")
        c, st = ac.expected(t, [b])
        rid = int(t.rule_id[idx])
        assert int(st["packets"][rid]) == 1 << 20 and int(st["bytes"][rid]) == 65535 << 20
        assert int(st["packets"].sum()) == 1 << 20 and int(c["pkts_dropped"][0]) == 1 << 20
