"""The refresh of known neighbours on the CPU: upe_neigh_patch_host (upe_rules.cpp, the exact twin
of upe_gpu_neigh_patch) and neigh.patch (numpy, on the slot arrays), over every table of
tests/neigh_cases.py small and embedded, with the records of tests/patch_cases.py.  The invariant
the device call rests on: a record whose address a probe reaches rewrites one slot's MAC and moves
nothing, so the patched snapshot answers as the snapshot compiled from the written tables does.
`make patch-san` runs the twin under the host sanitizers."""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np
import pytest

import neigh_cases as nc
import patch_cases as pc
import resolve_cases as rc
from upe_amd import gpu, neigh
from upe_amd.layout import ARP_DTYPE, CW_ARP, CW_NDP, NDP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = ["ip", "mac", "valid"]
NONE64 = (1 << 64) - 1


def _info(x):
    return tuple(int(x[f]) for f in ("records", "patched", "missed", "first_miss"))


def _check(name, arp, ndp, w):
    keys = rc.as_keys(pc.address_keys(name, w))
    # 1. the two twins agree
    image = gpu.NeighImage(arp, ndp)
    old = gpu.neigh_image_lookup_host(image, keys)
    assert np.array_equal(old, neigh.resolve_keys(arp, ndp, keys)), "the image before the patch"
    miss_h, info_h = gpu.neigh_patch_host(image, w)
    p_arp, p_ndp, miss_n, info_n = neigh.patch(arp, ndp, w)
    assert np.array_equal(miss_h, miss_n) and miss_h.dtype == miss_n.dtype
    assert _info(info_h) == info_n
    # 2. the misses are the records whose address the probe misses before the batch
    before = gpu.neigh_lookup_host(arp, ndp, rc.as_keys(pc.record_keys(w)))
    known = (w["kind"] == CW_ARP) | (w["kind"] == CW_NDP)
    want_held = known & (before != 0)
    assert np.array_equal(want_held, pc.held(arp, ndp, w)), "the probe model"
    assert np.array_equal(miss_h, np.nonzero(~want_held)[0])
    n, m = len(w), int((~want_held).sum())
    assert info_n == (n, n - m, m, int(miss_h[0]) if m else NONE64)
    # 3. the invariant: the held records through the reference's update, compiled again
    held = w[want_held]
    a2, n2 = arp.copy(), ndp.copy()
    assert gpu.neigh_apply_writes(a2, n2, held, now=99) == len(held)
    again = gpu.NeighImage(a2, n2)
    want = gpu.neigh_image_lookup_host(again, keys)
    got = gpu.neigh_image_lookup_host(image, keys)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: key {int(bad[0])}: {int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}"
    assert np.array_equal(want, neigh.resolve_keys(a2, n2, keys))
    # the missed records changed nothing: the held ones alone give the same image answers
    only = gpu.NeighImage(arp, ndp)
    miss_o, info_o = gpu.neigh_patch_host(only, held)
    assert len(miss_o) == 0 and _info(info_o) == (len(held), len(held), 0, NONE64)
    assert np.array_equal(gpu.neigh_image_lookup_host(only, keys), want)
    # 4. neigh.patch's arrays are the reference's (it does not model update_at)
    assert np.array_equal(p_arp[KEEP], a2[KEEP]) and np.array_equal(p_ndp[KEEP], n2[KEEP])
    for x in (image, again, only):
        x.free()
    return old, want, want_held


@pytest.mark.parametrize("name", pc.CASES)
def test_tables(name):
    cs, w = nc.case(name), pc.records(name)
    old, new, held = _check(name, cs.arp, cs.ndp, w)
    for fam, kind in (("arp", CW_ARP), ("ndp", CW_NDP)):
        an = nc.anatomy(cs.table(fam))
        mine = w["kind"] == kind
        if an["reachable"]:
            assert held[mine].any() and not np.array_equal(old, new), (name, fam)
        # each kind of address a probe does not reach is aimed at, and missed
        for k in an["hidden"] + an["stale"]:
            if k in cs.own(fam) or len(cs.table(fam)) <= 64:
                b = int(k).to_bytes(4, "little") + bytes(12) if fam == "arp" else k
                r = np.nonzero(mine & (w["ip"] == np.frombuffer(b, np.uint8)).all(axis=1))[0]
                assert len(r) and not held[r].any(), (name, fam, "unreached address held")
        # the absent addresses are missed (the zero address unless the table holds it)
        assert (~held[mine]).sum() >= pc.ABSENT // 2 - 1


def test_last_record_wins_and_second_slot_stays():
    """The address held in two slots: the slot the probe meets first takes the last record's MAC,
    the second slot keeps its own."""
    for fam, kind in (("arp", CW_ARP), ("ndp", CW_NDP)):
        t = nc.table(fam, "dup")
        k = nc.anatomy(t)["dup"][0]
        first = nc.Probe(t).slot(k)
        second = [s for s in range(len(t)) if s != first and t["valid"][s] and nc.key_at(t, s) == k]
        w = pc.make([(kind, k)] * 3)
        arp = t if fam == "arp" else np.zeros(0, ARP_DTYPE)
        ndp = t if fam == "ndp" else np.zeros(0, NDP_DTYPE)
        a, n, miss, info = neigh.patch(arp, ndp, w)
        out = a if fam == "arp" else n
        assert info == (3, 3, 0, NONE64) and len(miss) == 0
        assert out["mac"][first].tobytes() == pc.rank_mac(2)
        assert second and out["mac"][second[0]].tobytes() == t["mac"][second[0]].tobytes()
        image = gpu.NeighImage(arp, ndp)
        gpu.neigh_patch_host(image, w)
        key = rc.as_keys(rc.key_bytes([fam], [k], np.random.default_rng(1)))
        assert int(gpu.neigh_image_lookup_host(image, key)[0]) == rc.mac_word(pc.rank_mac(2))
        image.free()


@pytest.mark.parametrize("drop", ["arp", "ndp"])
def test_family_without_slots(drop):
    """One family's table has capacity 0: its records are all missed, the other's as before."""
    name = "combo"
    cs, w = nc.case(name), pc.records(name)
    arp = np.zeros(0, ARP_DTYPE) if drop == "arp" else cs.arp
    ndp = np.zeros(0, NDP_DTYPE) if drop == "ndp" else cs.ndp
    _, _, held = _check(name, arp, ndp, w)
    assert not held[w["kind"] == (CW_ARP if drop == "arp" else CW_NDP)].any()
    assert held[w["kind"] == (CW_NDP if drop == "arp" else CW_ARP)].any()


def test_empty_and_arguments():
    L = gpu.LIB
    cs = nc.case("combo")
    image = gpu.NeighImage(cs.arp, cs.ndp)
    miss, info = gpu.neigh_patch_host(image, pc.records("combo")[:0])
    assert len(miss) == 0 and _info(info) == (0, 0, 0, NONE64)
    info = np.zeros(1, gpu.PATCH_INFO_DTYPE)
    w = pc.records("combo").copy()
    assert L.upe_neigh_patch_host(None, w.ctypes.data, 1, None, info.ctypes.data) == -1
    assert L.upe_neigh_patch_host(image.ptr, w.ctypes.data, 1, None, None) == -1
    assert L.upe_neigh_patch_host(image.ptr, None, 1, None, info.ctypes.data) == -1
    assert L.upe_neigh_patch_host(image.ptr, w.ctypes.data, (1 << 32) - gpu.PATCH_BLOCK, None,
                                  info.ctypes.data) == -1
    assert b"32 bits" in L.upe_gpu_last_error()
    assert L.upe_neigh_image_lookup_host(None, None, 0, None) == -1
    # without a miss list the same info
    assert L.upe_neigh_patch_host(image.ptr, w.ctypes.data, len(w), None, info.ctypes.data) == 0
    assert _info(info[0])[0] == len(w) and _info(info[0])[1] + _info(info[0])[2] == len(w)
    image.free()


def test_patch_san_builds_and_passes():
    """The twin under the host sanitizers, as a stand-alone program (`make patch-san`)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "upe_amd", "csrc"), "patch-san",
                            f"BUILD={d}/"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "patch_san: ok" in r.stdout
