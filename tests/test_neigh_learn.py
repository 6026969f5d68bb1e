"""New neighbours learnt on the CPU: upe_neigh_learn_host (upe_rules.cpp, the exact twin of
upe_gpu_neigh_learn), neigh.learn (numpy) and the sequential model of tests/learn_cases.py, byte for
byte, over every case there; what each case must give is asserted here, so the parity tests cannot
pass by deferring everything.  The invariant the device call rests on: the learnt snapshot answers
as the reference's tables do after upe_neigh_apply_writes of the records that were not deferred,
and as the snapshot compiled from those tables does.  `make learn-san` runs the twin under the host
sanitizers."""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np
import pytest

import learn_cases as lc
import neigh_cases as nc
import resolve_cases as rc
from upe_amd import gpu, neigh
from upe_amd.layout import LEARN_INFO_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = LEARN_INFO_DTYPE.names
KEEP = ["ip", "mac", "valid"]


def _info(x):
    return tuple(int(x[f]) for f in FIELDS)


def _same_index(a, b):
    return a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and \
        np.array_equal(a[2], b[2])


@pytest.mark.parametrize("name", lc.CASES)
def test_cases(name):
    c = lc.case(name)
    image = c.image()
    before = image.read()
    # 1. the model gives what the case states
    want_index, want_defer, want_info, out = lc.model(before, c.recs)
    print(name, want_info)
    assert want_info[1:5] == c.expect, (name, want_info)
    assert sum(want_info[1:5]) == len(c.recs)
    if c.defer is None:
        assert want_info[4] == 0, "a case named for insertion defers"
    else:
        assert want_defer.tolist() == c.defer, "the records made to defer"
    # 2. the twins agree with it byte for byte
    defer_h, info_h = gpu.neigh_learn_host(image, c.recs)
    after = image.read()
    assert _info(info_h) == want_info
    assert np.array_equal(defer_h, want_defer) and defer_h.dtype == want_defer.dtype
    assert _same_index(after, want_index), "upe_neigh_learn_host's index"
    index_n, defer_n, info_n, arp_n, ndp_n = neigh.learn(before, c.recs, c.arp, c.ndp)
    assert info_n == want_info and np.array_equal(defer_n, want_defer)
    assert defer_n.dtype == np.uint32
    assert _same_index(index_n, want_index), "neigh.learn's index"
    # bits, seed and insertable are the compiled image's
    for f in ("arp_bits", "arp_seed", "ndp_bits", "ndp_seed", "arp_insertable", "ndp_insertable"):
        assert after[0][f] == before[0][f]
    # 3. the invariant: the records that were not deferred through the reference's update
    a2, n2 = lc.applied(c, want_defer)
    assert np.array_equal(arp_n[KEEP], a2[KEEP]) and np.array_equal(ndp_n[KEEP], n2[KEEP])
    keys = rc.as_keys(lc.keys(c))
    got = gpu.neigh_image_lookup_host(image, keys)
    want = gpu.neigh_lookup_host(a2, n2, keys)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{name}: key {int(bad[0])}: {int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}"
    again = gpu.NeighImage(a2, n2)
    assert np.array_equal(gpu.neigh_image_lookup_host(again, keys), want)
    # 4. the free counts are the applied arrays' invalid slots
    if want_info[4] == 0:
        assert want_info[6] == int((a2["valid"] == 0).sum())
        assert want_info[7] == int((n2["valid"] == 0).sum())
        assert (int(again.read()[0]["arp_free"]), int(again.read()[0]["ndp_free"])) == want_info[6:]
    if want_info[2]:
        assert not np.array_equal(got, gpu.neigh_image_lookup_host(c.image(), keys))
    for x in (image, again):
        x.free()


def test_later_mac_wins():
    c = lc.case("twice:wrap")
    image = c.image()
    gpu.neigh_learn_host(image, c.recs)
    got = gpu.neigh_image_lookup_host(image, rc.as_keys(lc.pc.record_keys(c.recs)))
    for r in range(4):
        assert int(got[r]) == rc.mac_word(lc.pc.rank_mac(2 + r % 2)), r
    image.free()


@pytest.mark.parametrize("name", nc.SMALL_CASES + ["embed:combo", "big4096"])
def test_room_zero_is_compile(name):
    cs = nc.case(name)
    a, b = gpu.NeighImage(cs.arp, cs.ndp), gpu.NeighImage(cs.arp, cs.ndp, room=(0, 0))
    assert _same_index(a.read(), b.read())
    info = a.read()[0]
    for fam in ("arp", "ndp"):
        t, an = cs.table(fam), nc.anatomy(cs.table(fam))
        valid = int((t["valid"] != 0).sum())
        assert int(info[fam + "_free"]) == len(t) - valid
        assert bool(info[fam + "_insertable"]) == (valid == len(an["reachable"]) and
                                                    int(info[fam + "_bits"]) != 0)
    a.free(), b.free()


def test_room_sizes_the_index():
    empty = gpu.NeighImage(None, None, room=(0, 5)).read()
    assert int(empty[0]["arp_bits"]) == 0 and not empty[0]["arp_insertable"]
    # 2^bits * 4 >= 5 * 5: a real index with no slot used
    assert int(empty[0]["ndp_bits"]) == 3 and empty[0]["ndp_insertable"]
    assert int(empty[0]["ndp_free"]) == 0 and not empty[2].any()
    t = lc.sparse("arp")
    for room, bits in ((0, 4), (4, 4), (5, 5), (1000, 11)):   # 8 keys: (8 + room) * 5 <= 4 << bits
        assert int(gpu.NeighImage(t, None, room=(room, 0)).read()[0]["arp_bits"]) == bits
    assert not gpu.LIB.upe_neigh_compile_room(None, 0, None, 0, (1 << 30) + 1, 0)
    assert b"room" in gpu.LIB.upe_gpu_last_error()


def test_empty_and_arguments():
    L = gpu.LIB
    c = lc.case("one_new:wrap")
    image = c.image()
    defer, info = gpu.neigh_learn_host(image, c.recs[:0])
    assert len(defer) == 0
    assert _info(info) == (0, 0, 0, 0, 0, lc.NONE64, 12, 12)
    info = np.zeros(1, LEARN_INFO_DTYPE)
    w = c.recs.copy()
    assert L.upe_neigh_learn_host(None, w.ctypes.data, 1, None, info.ctypes.data) == -1
    assert L.upe_neigh_learn_host(image.ptr, w.ctypes.data, 1, None, None) == -1
    assert L.upe_neigh_learn_host(image.ptr, None, 1, None, info.ctypes.data) == -1
    assert L.upe_neigh_learn_host(image.ptr, w.ctypes.data, (1 << 32) - gpu.LEARN_CHUNK, None,
                                  info.ctypes.data) == -1
    assert b"32 bits" in L.upe_gpu_last_error()
    assert L.upe_neigh_image_read(None, None, None, 0, None, 0) == -1
    buf = np.zeros(4, np.uint32)
    assert L.upe_neigh_image_read(image.ptr, None, buf.ctypes.data, 8, None, 0) == -1
    # without a defer list the same info
    assert L.upe_neigh_learn_host(image.ptr, w.ctypes.data, len(w), None, info.ctypes.data) == 0
    assert _info(info[0])[:5] == (2, 0, 2, 0, 0)
    image.free()


def test_learn_san_builds_and_passes():
    """The twin under the host sanitizers, as a stand-alone program (`make learn-san`)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "upe_amd", "csrc"), "learn-san",
                            f"BUILD={d}/"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "learn_san: ok" in r.stdout
