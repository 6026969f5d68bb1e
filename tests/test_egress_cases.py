"""CPU: the batches of tests/egress_cases.py forward what they claim, and the expected emit-mode
outputs derived from the restatement are consistent with the host's own readers of that layout.

Every batch's verdicts equal the kinds it was built from, at every table size and with both
neighbour tables; every lane pattern, every ordered pair of patterns and every tail shape occurs;
forwarded packets near each other have different records; expand_records over the expected raw
array gives back the per-packet records and upe_hdr_apply of those the restatement's frames;
upe_tx_flush_groups over the expected tx / tx_count (poison past every group's count) makes the
calls upe_tx_flush makes from the verdicts.  The comparison the GPU tests use
(egress_cases.check_layout) is shown to catch a record in slot i, a record in an unused slot, a
count left unwritten and two tx entries swapped, each named by group and slot.  After this,
tests/test_gpu_egress_cases.py trusts expected().
"""
from __future__ import annotations

import numpy as np
import pytest

import egress_cases as ec
from test_emit_records import records_from_reference
from upe_amd import gpu
from upe_amd.layout import V_FWD, VF_ARP_REPLY, desc_lens, desc_offsets

_EXP: dict = {}


def exp_of(name: str, nrules: int = 8, big: bool = False):
    key = (name, nrules, big)
    if key not in _EXP:
        b = ec.sequences()[name]
        _EXP[key] = ec.expected(ec.workload(b, ec.table(nrules), big))
    return _EXP[key]


def _rule_bits(t, kinds):
    idx = {ec.FWD4_HIT: "fwd4", ec.FWD4_MISS: "fwd4", ec.FWD6_HIT: "fwd6", ec.FWD6_MISS: "fwd6",
           ec.DROP_RULE: "drop", ec.DROP_ACTION: "action"}
    bits = np.zeros(len(kinds), np.uint32)
    for k, probe in idx.items():
        bits[kinds == k] = (t.probe_index[probe] + 1) << 8
    odd = np.arange(len(kinds)) % 2 == 1
    ttl1 = kinds == ec.TTL1
    bits[ttl1 & ~odd] = (t.probe_index["fwd4"] + 1) << 8
    bits[ttl1 & odd] = (t.probe_index["fwd6"] + 1) << 8
    return bits


@pytest.mark.parametrize("big", [False, True], ids=["lds", "memory"])
@pytest.mark.parametrize("nrules", ec.TABLE_SIZES)
def test_verdicts_equal_the_kinds(nrules, big):
    t = ec.table(nrules)
    assert sorted(t.probe_index.values()) == [0, nrules // 2 - 1, nrules // 2, nrules - 1]
    for name, b in ec.sequences().items():
        e = exp_of(name, nrules, big)
        want = ec.KIND_VERDICT[b.kinds] | _rule_bits(t, b.kinds)
        bad = np.nonzero(e.verdict != want)[0]
        assert bad.size == 0, (name, bad[:4], [ec.KIND_NAMES[k] for k in b.kinds[bad[:4]]],
                               [hex(v) for v in e.verdict[bad[:4]]])
        assert np.array_equal((e.verdict & 0xF) == V_FWD, b.fwd), name
        assert int(e.counters["pkts_forwarded"][0]) == int(b.fwd.sum()), name
        assert int(e.counters["pkts_in"][0]) == b.n, name


def test_tables_sit_where_the_kernels_branch():
    import accounting_cases as ac
    assert [ac.stats_path(n) for n in ec.TABLE_SIZES] == ["small", "mid", "group-by"]
    for big in (False, True):
        arp, ndp = ec.neighbours(big)
        assert len(arp) == len(ndp) == (8192 if big else 1024)
        reach = int(arp["valid"].sum())
        assert reach == int(ndp["valid"].sum()) == ec.NEIGH + (ec.BIG_FILL if big else 0)
        # the device index takes the least 2^bits slots with 4 * 2^bits >= 5 * entries: staged in
        # LDS up to 2048 slots (UPE_ARP_LDS_SLOTS)
        assert (5 * reach > 4 * 2048) == big


def test_every_pattern_pair_and_tail_occurs():
    pats = ec.patterns()
    assert list(pats) == ["empty", "full", "lane0", "lane63", "seam", "low", "high", "even", "odd",
                          "eighth", "seven_eighths"]
    assert [int(m.sum()) for m in list(pats.values())[:9]] == [0, 64, 1, 1, 2, 32, 32, 32, 32]
    seq = ec.sequences()
    fwd = seq["pairs"].fwd.reshape(-1, 64)
    which = [next(k for k, m in pats.items() if np.array_equal(m, g)) for g in fwd]
    assert which == ec.pair_order()
    pairs = set(zip(which[:-1], which[1:]))
    assert pairs == {(a, b) for a in pats for b in pats} and len(which) == 122
    # in every whole group with room for it, every kind that does not forward sits somewhere
    k = seq["pairs"].kinds.reshape(-1, 64)
    for g in range(len(k)):
        if 64 - fwd[g].sum() >= 2 * len(ec.OTHER_KINDS) - 1:
            assert set(ec.OTHER_KINDS) <= set(k[g].tolist()), g
    assert set(range(11)) == set(seq["pairs"].kinds.tolist())
    whole = seq["pairs"].n - 64
    for n in ec.SMALL_CUTS + tuple(whole + r for r in ec.TAIL_EXTRA):
        for tag, count in (("last", 1), ("none", 0)):
            b = seq[f"cut:{n}:{tag}"]
            tail = b.fwd[(n - 1) // 64 * 64:]
            assert b.n == n and int(tail.sum()) == count and bool(tail[-1]) == bool(count)
            assert np.array_equal(b.fwd[:(n - 1) // 64 * 64], seq["pairs"].fwd[:(n - 1) // 64 * 64])
    assert not seq["all_empty"].fwd.any() and seq["all_full"].fwd.all()
    assert seq["all_empty"].n % 64 and seq["all_full"].n > 4 * 64


def test_records_differ_between_neighbours():
    for name in ec.sequences():
        e = exp_of(name)
        ec.assert_unique(e.records)          # (expected() has asserted it already)
        fwd = e.records[:, 15] != 0
        assert np.array_equal(fwd, (e.verdict & 0xF) == V_FWD)
    e = exp_of("pairs")
    twin = e.records.copy()
    i, j = np.nonzero(twin[:, 15] == 4)[0][[3, 4]]
    twin[j] = twin[i]
    with pytest.raises(AssertionError, match="share a record"):
        ec.assert_unique(twin)
    # a hit carries the neighbour's and the port's MAC, a miss the frame's own (its index)
    b = ec.sequences()["pairs"]
    offs = desc_offsets(b.desc)
    miss = np.nonzero(np.isin(b.kinds, (ec.FWD4_MISS, ec.FWD6_MISS)))[0]
    assert np.array_equal(e.records[miss, :12], b.frames[offs[miss, None] + np.arange(12)])
    hit = np.nonzero(np.isin(b.kinds, (ec.FWD4_HIT, ec.FWD6_HIT)))[0]
    assert (e.records[hit, 0] == 0x02).all() and (e.records[hit, 1] >= 0xE4).all()
    assert len(np.unique(e.records[hit, 5])) == ec.NEIGH


def test_vectorised_records_equal_the_definition():
    """records_from_reference packet by packet, as the format's comment reads."""
    b = ec.sequences()["pairs"]
    e = exp_of("pairs")
    offs = desc_offsets(b.desc)
    for i in range(b.n):
        want = np.zeros(16, np.uint8)
        if (e.verdict[i] & 0xF) == V_FWD:
            out = e.frames_applied[offs[i]:offs[i] + 26]
            want[:12] = out[:12]
            if b.frames[offs[i] + 12] == 0x86:
                want[12], want[15] = out[21], 6
            else:
                want[12], want[13], want[14], want[15] = out[22], out[24], out[25], 4
        assert np.array_equal(e.records[i], want), i


@pytest.mark.parametrize("big", [False, True], ids=["lds", "memory"])
def test_expected_layout_reads_back(big):
    for name, b in ec.sequences().items():
        e = exp_of(name, 8, big)
        assert e.raw.shape == (b.n + ec.CANARY, 16) and e.tx.shape == (b.n + ec.CANARY,)
        assert np.array_equal(gpu.expand_records(e.raw, e.verdict), e.records), name
        assert np.array_equal(gpu.hdr_apply(e.frames, b.desc, e.records), e.frames_applied), name
        # the slots not named by record_slots hold poison, in all three arrays
        used = np.zeros(b.n + ec.CANARY, bool)
        used[e.slots[b.fwd]] = True
        assert (e.raw[~used] == ec.POISON).all() and (e.raw[used, 15] != ec.POISON).all()
        assert (e.tx[~used] == ec.POISON32).all()
        assert np.array_equal(e.tx[used], e.fwd_list), name
        assert np.array_equal(e.tx_count[:e.groups], b.fwd[:e.groups * 64 - 64].reshape(-1, 64)
                              .sum(axis=1).tolist() + [int(b.fwd[e.groups * 64 - 64:].sum())])
        assert (e.tx_count[e.groups:] == ec.POISON32).all()
        # emit mode leaves the frames alone but for the answered ARP requests' first 48 bytes
        diff = np.nonzero(e.frames != b.frames)[0]
        offs = desc_offsets(b.desc)
        arp = np.nonzero(e.verdict & VF_ARP_REPLY)[0]
        assert np.array_equal(arp, np.nonzero(b.kinds == ec.ARP_REPLY)[0])
        owner = np.searchsorted(offs, diff, side="right") - 1
        assert np.isin(owner, arp).all() and (diff - offs[owner] < 48).all(), name
        assert len(arp) == 0 or len(diff) > 0


@pytest.mark.parametrize("burst", [1, 7, 32, 64])
def test_flush_groups_makes_the_calls_of_flush(burst):
    for name in ("pairs", "all_empty", "all_full", "cut:65:last", "cut:7775:none", "cut:1:last"):
        b = ec.sequences()[name]
        e = exp_of(name)
        want = gpu.tx_flush(e.frames_applied, b.desc, e.verdict, burst)
        got = gpu.tx_flush(e.frames_applied, b.desc, None, burst, groups=(e.tx, e.tx_count))
        assert want[1:] == got[1:] == (int(b.fwd.sum()), 0), name
        assert len(want[0]) == len(got[0]), name
        for (wi, wd), (gi, gd) in zip(want[0], got[0]):
            assert np.array_equal(wi, gi) and wd == gd, name   # same frames (pointers), same bytes
        assert np.array_equal(np.concatenate([i for i, _ in got[0]] or [np.zeros(0, np.int64)]),
                              e.fwd_list), name
        lens = desc_lens(b.desc)
        assert all(len(d) == lens[i] for idx, data in got[0] for i, d in zip(idx, data))


def test_three_passes_share_descriptors():
    p = ec.three_passes()
    assert len({b.fwd.tobytes() for b in p}) == 3
    for b in p[1:]:
        assert np.array_equal(b.desc, p[0].desc) and not np.array_equal(b.frames, p[0].frames)
    # a slot only an earlier pass forwarded into exists (the later pass leaves it alone)
    t = ec.table(8)
    e = [ec.expected(ec.workload(b, t)) for b in p]
    only_first = (e[0].raw[:, 15] != ec.POISON) & (e[2].raw[:, 15] == ec.POISON)
    assert only_first.sum() > 100


# ---------------------------------------------------------------------------------------------
# the comparison catches what it is there for
# ---------------------------------------------------------------------------------------------

def _broken(name="pairs"):
    e = exp_of(name)
    return e, e.raw.copy(), e.tx.copy(), e.tx_count.copy()


def test_check_accepts_the_expected_arrays():
    e, raw, tx, cnt = _broken()
    ec.check_expected(e, "same", raw=raw, tx=tx, tx_count=cnt)
    ec.check_expected(e, "same", raw=raw.reshape(-1))


def test_check_catches_a_record_in_slot_i():
    """Layout 1's mistake: a forwarded packet's record at its own index, not its rank."""
    e, raw, _, _ = _broken()
    i = int(next(i for i in e.fwd_list if e.slots[i] != i and not (e.verdict[e.slots[i]] & 0xF) == V_FWD
                 and e.raw[i, 15] == ec.POISON))
    raw[i] = e.records[i]
    raw[e.slots[i]] = ec.POISON
    first = min(i, int(e.slots[i]))
    with pytest.raises(AssertionError, match=rf"group {first // 64} slot {first} \(lane {first % 64}\)"):
        ec.check_expected(e, "moved", raw=raw)


def test_check_catches_an_extra_record():
    e, raw, _, _ = _broken()
    g = ec.pair_order().index("lane0")
    s = 64 * g + 1                      # the slot after the group's only record
    assert e.raw[s, 15] == ec.POISON and e.raw[s - 1, 15] != ec.POISON
    raw[s] = 0                          # what layout 1 wrote for a packet not forwarded
    with pytest.raises(AssertionError, match=rf"group {g} slot {s} .*want no record"):
        ec.check_expected(e, "extra", raw=raw)
    raw = e.raw.copy()
    raw[e.n] = e.records[e.fwd_list[0]]     # the canary behind the last group
    with pytest.raises(AssertionError, match=rf"group {e.n // 64} slot {e.n} "):
        ec.check_expected(e, "canary", raw=raw)


def test_check_catches_a_count_left_unwritten():
    e, _, tx, cnt = _broken()
    g = ec.pair_order().index("empty")
    assert cnt[g] == 0
    cnt[g] = ec.POISON32
    with pytest.raises(AssertionError, match=rf"tx_count .* group {g} \(slot {64 * g}\): want 0x0"):
        ec.check_expected(e, "unwritten", tx=tx, tx_count=cnt)


def test_check_catches_a_swap_within_a_group():
    e, _, tx, cnt = _broken()
    g = ec.pair_order().index("seam")
    s = 64 * g
    assert cnt[g] == 2 and tx[s:s + 2].tolist() == [s + 31, s + 32]
    tx[s], tx[s + 1] = tx[s + 1], tx[s]
    with pytest.raises(AssertionError, match=rf"tx differs in 2 entries, first in group {g} slot {s} "):
        ec.check_expected(e, "swapped", tx=tx, tx_count=cnt)
