"""CPU: next hops per flow key.  The numpy mirror (upe_amd/neigh.py, the expected value of
tests/test_gpu_resolve.py) and the library's host twin (upe_neigh_lookup_host) against the pinned
probe model of tests/neigh_cases.py and, where it is built, against the reference's own
arp_get_mac / ndp_get_mac over tables made by arp_table_init / ndp_table_init; the compile half
of the snapshot (upe_neigh_compile); `make resolve-san`.  Bit for bit throughout."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import neigh_cases as nc
import oracle
import resolve_cases as rc
from upe_amd import gpu, neigh
from upe_amd.layout import ARP_DTYPE, NDP_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "upe_amd", "csrc")
NEW_SYMBOLS = ("upe_neigh_compile", "upe_neigh_image_free", "upe_gpu_load_neigh_image",
               "upe_gpu_resolve_keys", "upe_neigh_lookup_host")


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(gpu.LIB_PATH)
    assert not [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
    assert set(NEW_SYMBOLS) <= set(gpu.EXPORTED)


@pytest.mark.parametrize("name", rc.CASES)
def test_twins_equal_the_probe_model(name):
    cs = nc.case(name)
    kb, fams, addrs, groups = rc.queries(name)
    want = rc.probe_words(cs, fams, addrs)
    keys = rc.as_keys(kb)
    for what, got in (("neigh.resolve_keys", neigh.resolve_keys(cs.arp, cs.ndp, keys)),
                      ("upe_neigh_lookup_host", gpu.neigh_lookup_host(cs.arp, cs.ndp, keys))):
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{name} {what}: {bad.size} of {len(want)} differ, first "
                               f"{int(bad[0])} ({fams[bad[0]]} {groups[bad[0]]}): "
                               f"{int(got[bad[0]]):#x} vs {int(want[bad[0]]):#x}")
    # the queries reach what the case is about: hits wherever anything is reachable, and every
    # flipped address misses
    g = np.array(groups)
    for fam in ("arp", "ndp"):
        f = np.array(fams) == fam
        if nc.anatomy(cs.table(fam))["reachable"]:
            assert (want[f & (g == "stored")] != 0).any(), (name, fam)
            assert (g[f] == "flip").sum() >= 24, (name, fam)
        assert not want[f & (g == "flip")].any(), (name, fam)
    assert not (want >> np.uint64(49)).any()


class _RefTable(ctypes.Structure):
    """arp_table_t / ndp_table_t (reference include/arp_table.h:20-24): the two fields read here,
    and room for the lock."""
    _fields_ = [("entries", ctypes.c_void_p), ("capacity", ctypes.c_size_t),
                ("lock", ctypes.c_uint8 * 256)]


def _ref_answers(lib, cs, fams, addrs):
    """The reference's own lookups over tables made by its init functions, the case's slot arrays
    copied into `entries`."""
    tabs = {}
    for fam, init in (("arp", lib.arp_table_init), ("ndp", lib.ndp_table_init)):
        src = np.ascontiguousarray(cs.table(fam))
        if len(src) == 0:
            continue   # (the reference has no table of no slots)
        t = _RefTable()
        init.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
        assert init(ctypes.byref(t), len(src)) == 0 and t.capacity == len(src)
        ctypes.memmove(t.entries, src.ctypes.data, src.nbytes)
        tabs[fam] = t
    lib.arp_get_mac.restype = lib.ndp_get_mac.restype = ctypes.c_bool
    lib.arp_get_mac.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.ndp_get_mac.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p]
    mac = (ctypes.c_uint8 * 6)()
    out = np.zeros(len(fams), np.uint64)
    for i, (f, a) in enumerate(zip(fams, addrs)):
        if f not in tabs:
            continue
        get = lib.arp_get_mac if f == "arp" else lib.ndp_get_mac
        if get(ctypes.byref(tabs[f]), a, mac):
            out[i] = rc.mac_word(bytes(mac))
    for fam, t in tabs.items():
        (lib.arp_table_destroy if fam == "arp" else lib.ndp_table_destroy)(ctypes.byref(t))
    return out


@pytest.mark.parametrize("name", rc.CASES)
def test_twins_equal_the_reference(name):
    if not oracle.ref_available():
        return   # (as tests/test_neigh_cases.py: the reference harness is built where its source is)
    assert ARP_DTYPE.itemsize == 32 and NDP_DTYPE.itemsize == 40   # arp_entry_t / ndp_entry_t
    cs = nc.case(name)
    kb, fams, addrs, _ = rc.queries(name)
    want = _ref_answers(oracle.ref_lib(), cs, fams, addrs)
    keys = rc.as_keys(kb)
    assert np.array_equal(neigh.resolve_keys(cs.arp, cs.ndp, keys), want), name
    assert np.array_equal(gpu.neigh_lookup_host(cs.arp, cs.ndp, keys), want), name


def test_other_ip_versions_find_nothing():
    cs = nc.case("combo")
    rng = np.random.default_rng(3)
    a4 = next(iter(nc.anatomy(cs.arp)["reachable"]))
    a6 = next(iter(nc.anatomy(cs.ndp)["reachable"]))
    fams = [4, 6, 0, 5, 255, 0, 5, 255]
    addrs = [a4, a6, a4, a4, a4, a6, a6, a6]
    keys = rc.as_keys(rc.key_bytes(fams, addrs, rng))
    for got in (neigh.resolve_keys(cs.arp, cs.ndp, keys),
                gpu.neigh_lookup_host(cs.arp, cs.ndp, keys)):
        assert got[0] and got[1] and not got[2:].any(), got


def test_ipv4_union_bytes_4_to_15_are_not_read():
    name = "embed:combo"
    cs = nc.case(name)
    _, fams, addrs, _ = rc.queries(name)
    fams, addrs = fams[:600], addrs[:600]
    dirty = rc.key_bytes(fams, addrs, np.random.default_rng(4))
    clean = rc.key_bytes(fams, addrs, np.random.default_rng(4), clean4=True)
    v4 = np.array(fams) == "arp"
    assert dirty[v4, 24:36].any() and not clean[v4, 24:36].any()
    want = rc.probe_words(cs, fams, addrs)
    assert want[v4].any()
    for k in (dirty, clean):
        assert np.array_equal(neigh.resolve_keys(cs.arp, cs.ndp, rc.as_keys(k)), want)
        assert np.array_equal(gpu.neigh_lookup_host(cs.arp, cs.ndp, rc.as_keys(k)), want)


def test_lookup_host_argument_errors():
    L = gpu.LIB
    t = np.zeros(3, ARP_DTYPE)
    out = np.zeros(1, np.uint64)
    k = rc.as_keys(rc.key_bytes([4], [1], np.random.default_rng(0)))
    assert L.upe_neigh_lookup_host(t.ctypes.data, 3, None, 0, k.ctypes.data, 1, out.ctypes.data) == -1
    assert b"power of two" in L.upe_host_last_error()
    assert L.upe_neigh_lookup_host(None, 4, None, 0, k.ctypes.data, 1, out.ctypes.data) == -1
    assert b"null" in L.upe_host_last_error()
    assert L.upe_neigh_lookup_host(None, 0, None, 0, None, 1, out.ctypes.data) == -1
    assert L.upe_neigh_lookup_host(None, 0, None, 0, None, 0, None) == 0
    assert L.upe_neigh_lookup_host(None, 0, None, 0, k.ctypes.data, 1, out.ctypes.data) == 0
    assert out[0] == 0


# ---------------------------------------------------------------------------------------------
# upe_neigh_compile
# ---------------------------------------------------------------------------------------------

def test_compile_one_fold_three_and_four():
    three, four = nc._one_fold("ndp", 3), nc._one_fold("ndp", 4)
    assert len(nc.anatomy(four)["reachable"]) == 4
    gpu.NeighImage(nc.table("arp", "dup"), three).free()
    with pytest.raises(gpu.UpeGpuError, match="placement"):
        gpu.NeighImage(nc.table("arp", "dup"), four)
    assert b"fold_v6" in gpu.LIB.upe_gpu_last_error()


def test_compile_checks_its_arguments_as_load_neigh_does():
    L = gpu.LIB
    t = np.zeros(16, ARP_DTYPE)
    assert not L.upe_neigh_compile(t.ctypes.data, 12, None, 0)
    assert b"power of two" in L.upe_gpu_last_error()
    assert not L.upe_neigh_compile(None, 0, None, 16)
    assert b"null table" in L.upe_gpu_last_error()
    im = L.upe_neigh_compile(None, 0, None, 0)
    assert im
    L.upe_neigh_image_free(im)
    L.upe_neigh_image_free(None)


# What the image holds is the library's own business (struct upe_neigh_image, upe_rules.h), so
# that equal tables give equal images is checked from inside: a C++ program over the internal
# header, linked with the compiler's source.
EQUAL_IMAGES = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "upe_rules.h"
extern "C" int upe_gpu_set_last_error(const char* m) { fprintf(stderr, "%s\n", m); return -1; }
static bool same(const std::vector<uint4>& a, const std::vector<uint4>& b) {
    return a.size() == b.size() && memcmp(a.data(), b.data(), a.size() * sizeof(uint4)) == 0;
}
static bool equal(const upe_neigh_image* a, const upe_neigh_image* b) {
    return same(a->im.arp, b->im.arp) && same(a->im.ndp, b->im.ndp) &&
           a->im.arp_bits == b->im.arp_bits && a->im.arp_seed == b->im.arp_seed &&
           a->im.ndp_bits == b->im.ndp_bits && a->im.ndp_seed == b->im.ndp_seed;
}
int main(int argc, char** argv) {
    // argv[1]: the two slot arrays as the test wrote them (ARP entries, then NDP entries)
    const size_t na = 4096, nn = 4096;
    std::vector<upe_arp_entry_t> arp(na), arp2;
    std::vector<upe_ndp_entry_t> ndp(nn), ndp2;
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f || fread(arp.data(), sizeof arp[0], na, f) != na ||
        fread(ndp.data(), sizeof ndp[0], nn, f) != nn)
        return fprintf(stderr, "no input\n"), 2;
    fclose(f);
    arp2 = arp, ndp2 = ndp;   // equal tables at other addresses
    upe_neigh_image* a = upe_neigh_compile(arp.data(), na, ndp.data(), nn);
    upe_neigh_image* b = upe_neigh_compile(arp2.data(), na, ndp2.data(), nn);
    // update_at is not part of a snapshot
    for (auto& e : arp2) e.update_at += 77;
    upe_neigh_image* c = upe_neigh_compile(arp2.data(), na, ndp2.data(), nn);
    // another MAC in a reachable entry (argv[2]: its slot) is
    arp2[argc > 2 ? strtoul(argv[2], nullptr, 10) % na : 0].mac[5] ^= 1;
    upe_neigh_image* d = upe_neigh_compile(arp2.data(), na, ndp2.data(), nn);
    if (!a || !b || !c || !d) return 3;
    const int bad = !equal(a, b) | !equal(a, c) << 1 | equal(a, d) << 2 |
                    (a->im.arp_bits < 11) << 3 | (a->im.ndp_bits < 11) << 4;
    upe_neigh_image_free(a), upe_neigh_image_free(b), upe_neigh_image_free(c);
    upe_neigh_image_free(d);
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
"""


def test_compile_gives_equal_images_for_equal_tables():
    arp, ndp = nc.table("arp", "big4096"), nc.table("ndp", "big4096")
    with tempfile.TemporaryDirectory() as d:
        src, exe, data = (os.path.join(d, x) for x in ("eq.cpp", "eq", "tables.bin"))
        open(src, "w").write(EQUAL_IMAGES)
        with open(data, "wb") as f:
            f.write(np.ascontiguousarray(arp).tobytes())
            f.write(np.ascontiguousarray(ndp).tobytes())
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-I", CSRC, "-o", exe, src,
                        os.path.join(CSRC, "upe_rules.cpp")], check=True)
        slot = next(iter(nc.anatomy(arp)["reachable"].values()))
        r = subprocess.run([exe, data, str(slot)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_make_resolve_san_runs_clean():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["make", "-C", CSRC, "resolve-san", f"BUILD={d}/"],
                           capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "resolve_san: ok" in r.stdout
