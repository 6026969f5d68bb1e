"""The ingress batch on the host: the ABI of upe_gpu_ingress_gather (include/upe_gpu.h: struct
layouts against the numpy mirrors, the export, the clean failure without a context) and
ingress.gather_host, the numpy restatement of its rules, against the golden fixtures — frames
scattered over a pktbuf pool come back byte for byte, classify to the reference's verdicts, and
the control positions are the ones is_table_write's rule gives — and against hand-written cases
of the capacity, bad-handle and empty-burst rules.  No GPU: the device side is
tests/test_gpu_ingress_gather.py."""
from __future__ import annotations

import dataclasses
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import golden_io
import oracle
from upe_amd import gpu, ingress, layout
from upe_amd.layout import FRAME_TAIL, HDR_WINDOW, desc_lens, desc_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["config_a", "config_c_small", "edge_zero", "edge_consistent", "ndp_walk"]
STRIDE = 2064
NONE = 2**64 - 1

C_LAYOUT = r"""
#include <stdio.h>
#include "upe_gpu.h"
#define S(t) printf(#t " %zu\n", sizeof(t))
#define P(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  S(upe_pktbuf_t); P(upe_pktbuf_t, timestamp); P(upe_pktbuf_t, len); P(upe_pktbuf_t, data);
  S(upe_ingress_info_t);
  P(upe_ingress_info_t, packets); P(upe_ingress_info_t, packed); P(upe_ingress_info_t, bytes);
  P(upe_ingress_info_t, need); P(upe_ingress_info_t, bad); P(upe_ingress_info_t, first_bad);
  P(upe_ingress_info_t, n_ctrl); P(upe_ingress_info_t, first_ctrl);
  printf("UPE_INGRESS_BLOCK %d\n", UPE_INGRESS_BLOCK);
  printf("UPE_PKTBUF_DATA %d\n", UPE_PKTBUF_DATA);
  printf("modes %d\n", UPE_INGRESS_REF + 10 * UPE_INGRESS_WINDOW + 100 * UPE_INGRESS_FULL);
  return 0;
}
"""


def test_struct_layouts_match_numpy_mirrors():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write(C_LAYOUT)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-I",
                        os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in out.strip().splitlines())}
    for name, dt in (("upe_pktbuf_t", layout.PKTBUF_DTYPE),
                     ("upe_ingress_info_t", layout.INGRESS_INFO_DTYPE)):
        assert got[name] == dt.itemsize
        for f in dt.names:
            assert got[f"{name}.{f}"] == dt.fields[f][1], (name, f)
    assert layout.PKTBUF_DTYPE.itemsize == 2064 and layout.INGRESS_INFO_DTYPE.itemsize == 64
    assert got["UPE_INGRESS_BLOCK"] == gpu.INGRESS_BLOCK
    assert got["UPE_PKTBUF_DATA"] == layout.PKTBUF_DATA
    assert got["modes"] == gpu.INGRESS_REF + 10 * gpu.INGRESS_WINDOW + 100 * gpu.INGRESS_FULL
    assert (gpu.INGRESS_REF, gpu.INGRESS_WINDOW, gpu.INGRESS_FULL) == \
        (ingress.REF, ingress.WINDOW, ingress.FULL)


def test_library_exports_the_call():
    assert "upe_gpu_ingress_gather" in gpu.EXPORTED
    assert hasattr(gpu.LIB, "upe_gpu_ingress_gather")
    assert hasattr(gpu.LIB, "upe_gpu_ingress_gather_timed")   # the timing tool's, not in the header
    assert "upe_gpu_ingress_gather_timed" not in open(
        os.path.join(ROOT, "include", "upe_gpu.h")).read()


def test_call_without_a_context_fails_cleanly():
    """-1 and a message, no crash: no context can exist without a GPU, and a NULL one is refused
    before anything is touched."""
    pool = np.zeros(4 * 128, np.uint8)
    slot = np.zeros(4, np.uint32)
    desc = np.zeros(4, np.uint64)
    info = np.full(64, 0xA5, np.uint8)
    rc = gpu.LIB.upe_gpu_ingress_gather(None, pool.ctypes.data, pool.size, 128, slot.ctypes.data,
                                        4, ingress.REF, None, 0, desc.ctypes.data, None, None,
                                        info.ctypes.data, None)
    assert rc == -1
    assert gpu.LIB.upe_gpu_last_error().decode().strip()
    assert np.all(info == 0xA5) and not desc.any()


# ---- gather_host against the goldens ---------------------------------------------------------

def frames_of(wl):
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    return [wl.frames[o:o + ln] for o, ln in zip(offs, lens)], lens


def table_write_positions(frames, lens):
    """is_table_write (upe_worker.c) / upe_ctrl_mark's rule, one frame at a time, independent of
    ingress.table_writes."""
    out = []
    for k, (f, ln) in enumerate(zip(frames, lens)):
        b = bytes(f[:ln]) + bytes(64)
        et = b[12] << 8 | b[13]
        if et == 0x0806:
            hit = b[14:20] == bytes([0, 1, 8, 0, 6, 4])
        else:
            hit = et == 0x86DD and ln >= 78 and b[20] == 58 and b[54] in (135, 136)
        if hit:
            out.append(k)
    return np.array(out, np.uint32)


@functools.lru_cache(maxsize=None)
def scattered(case):
    """The case's frames in a pool twice as large, at a random permutation of slots; the pool's
    other bytes, stale data past each frame included, are 0xEE."""
    wl, ref = golden_io.load(case)
    frames, lens = frames_of(wl)
    rng = np.random.default_rng(len(case) * 1000 + wl.n)
    slots = rng.permutation(2 * wl.n)[:wl.n].astype(np.uint32)
    ts = rng.integers(1, 1 << 62, wl.n, dtype=np.uint64)
    pool = ingress.make_pool(frames, lens, slots, 2 * wl.n, STRIDE, ts, fill=0xEE)
    for a in (pool, slots, ts):
        a.setflags(write=False)
    return wl, ref, frames, lens, pool, slots, ts


@pytest.mark.parametrize("case", CASES)
def test_gather_host_full_gives_the_frames_back(case):
    wl, ref, frames, lens, pool, slots, ts = scattered(case)
    out, desc, got_ts, ctrl, info = ingress.gather_host(pool, STRIDE, slots, ingress.FULL)
    assert int(info["packets"]) == int(info["packed"]) == wl.n == len(desc)
    assert int(info["bytes"]) == int(info["need"]) == out.size
    assert int(info["bad"]) == 0 and int(info["first_bad"]) == NONE
    assert np.array_equal(got_ts, ts)
    po, pl = desc_offsets(desc), desc_lens(desc)
    at = 0
    for k in range(wl.n):
        assert po[k] == at and pl[k] == lens[k], k
        assert np.array_equal(out[at:at + lens[k]], frames[k]), f"frame {k} differs"
        end = at + ((int(lens[k]) + 15) & ~15)
        assert not out[at + lens[k]:end].any(), f"pad after frame {k} is not zero"
        at = end
    assert at == out.size
    want_ctrl = table_write_positions(frames, lens)
    assert np.array_equal(ctrl, want_ctrl)
    assert int(info["n_ctrl"]) == want_ctrl.size
    assert int(info["first_ctrl"]) == (int(want_ctrl[0]) if want_ctrl.size else NONE)
    if case in ("edge_zero", "edge_consistent", "ndp_walk"):
        assert want_ctrl.size > 0
    # the gathered batch classifies to the reference's verdicts
    again = dataclasses.replace(wl, frames=np.concatenate([out, np.zeros(FRAME_TAIL, np.uint8)]),
                                desc=desc)
    r = oracle.run_restated(again, apply_control=True)
    assert np.array_equal(r.verdict, ref["verdict"])
    assert r.counters.tobytes() == np.asarray(ref["counters"]).tobytes()


@pytest.mark.parametrize("case", CASES)
def test_gather_host_ref_and_window(case):
    wl, ref, frames, lens, pool, slots, ts = scattered(case)
    full = ingress.gather_host(pool, STRIDE, slots, ingress.FULL)
    out, desc, got_ts, ctrl, info = ingress.gather_host(pool, STRIDE, slots, ingress.REF)
    assert out.size == 0 and int(info["bytes"]) == int(info["need"]) == 0
    assert np.array_equal(desc_offsets(desc), slots.astype(np.int64) * STRIDE + 16)
    assert np.array_equal(desc_lens(desc), lens)
    assert np.array_equal(ctrl, full[3]) and np.array_equal(got_ts, ts)
    # classified where the frames lie in the pool
    inplace = dataclasses.replace(wl, frames=pool.copy(), desc=desc)
    r = oracle.run_restated(inplace, apply_control=True)
    assert np.array_equal(r.verdict, ref["verdict"])
    out, desc, got_ts, ctrl, info = ingress.gather_host(pool, STRIDE, slots, ingress.WINDOW)
    assert out.size == wl.n * HDR_WINDOW == int(info["bytes"]) == int(info["need"])
    assert int(info["packed"]) == wl.n
    assert np.array_equal(desc_offsets(desc), np.arange(wl.n) * HDR_WINDOW)
    assert np.array_equal(desc_lens(desc), lens)
    assert np.array_equal(ctrl, full[3]) and np.array_equal(got_ts, ts)
    for k in range(wl.n):
        m = min(int(lens[k]), HDR_WINDOW)
        w = out[k * HDR_WINDOW:(k + 1) * HDR_WINDOW]
        assert np.array_equal(w[:m], frames[k][:m]) and not w[m:].any(), k


# ---- hand-written cases ----------------------------------------------------------------------

def small_pool():
    """stride 128 (112 data bytes), 6 buffers; frame k = bytes k+1, lengths 0, 1, 16, 17, 112."""
    lens = [0, 1, 16, 17, 112]
    frames = [np.full(112, k + 1, np.uint8) for k in range(5)]   # stale data past len
    return ingress.make_pool(frames, lens, [4, 0, 3, 1, 5], 6, 128, [10, 11, 12, 13, 14]), lens


def test_capacity_rule():
    pool, lens = small_pool()
    slots = np.array([4, 0, 3, 1, 5], np.uint32)
    out, desc, ts, ctrl, info = ingress.gather_host(pool, 128, slots, ingress.FULL)
    assert desc_offsets(desc).tolist() == [0, 0, 16, 32, 64] and int(info["need"]) == 176
    assert ts.tolist() == [10, 11, 12, 13, 14]
    assert out[:16].tolist() == [2] + [0] * 15 and out[32:64].tolist() == [4] * 17 + [0] * 15
    #          cap: (packed, bytes)
    for cap, (packed, used) in {0: (1, 0), 15: (1, 0), 16: (2, 16), 63: (3, 32), 64: (4, 64),
                                175: (4, 64), 176: (5, 176), 4096: (5, 176)}.items():
        o, d, t, c, inf = ingress.gather_host(pool, 128, slots, ingress.FULL, out_bytes=cap)
        assert (int(inf["packed"]), int(inf["bytes"]), int(inf["need"])) == (packed, used, 176), cap
        assert len(d) == len(t) == packed and np.array_equal(o, out[:used])
        assert np.array_equal(d, desc[:packed])
    with pytest.raises(ValueError):
        ingress.gather_host(pool, 128, slots, ingress.WINDOW, out_bytes=5 * 96 - 1)
    assert ingress.gather_host(pool, 128, slots, ingress.WINDOW, out_bytes=5 * 96)[0].size == 480


def test_bad_handles():
    pool, lens = small_pool()
    pool = pool.copy()
    head = pool.view("<u8")
    head[(2 * 128 + 8) // 8] = 113              # buffer 2: len = stride - 15
    slots = np.array([4, 6, 0, 2, 3, 0xFFFFFFFF], np.uint32)   # 6: one past the last buffer
    for mode in (ingress.REF, ingress.WINDOW, ingress.FULL):
        out, desc, ts, ctrl, info = ingress.gather_host(pool, 128, slots, mode)
        assert (int(info["bad"]), int(info["first_bad"])) == (3, 1)
        assert int(info["packed"]) == 6 and desc_lens(desc).tolist() == [0, 0, 1, 0, 16, 0]
        assert ts.tolist() == [10, 0, 11, 0, 12, 0]   # buffer 2 was never filled: timestamp 0
        offs = desc_offsets(desc).tolist()
        if mode == ingress.REF:
            assert offs == [4 * 128 + 16, 16, 16, 16, 3 * 128 + 16, 16]
        elif mode == ingress.WINDOW:
            assert offs == [0, 96, 192, 288, 384, 480] and not out[96:192].any()
        else:
            assert offs == [0, 16, 0, 16, 16, 16] and int(info["bytes"]) == 32
    # len is compared as 64 bits: 2^32 + 64 is bad, not 64; 65536 is bad whatever the stride
    big = ingress.make_pool([np.zeros(64, np.uint8)] * 3, [2**32 + 64, 65536, 65535], [0, 1, 2], 3,
                            131088)
    out, desc, ts, ctrl, info = ingress.gather_host(big, 131088, [0, 1, 2], ingress.FULL)
    assert desc_lens(desc).tolist() == [0, 0, 65535] and int(info["bad"]) == 2
    assert int(info["need"]) == 65536


def test_control_marks_read_zero_past_len():
    arp = np.zeros(64, np.uint8)
    arp[12:20] = [0x08, 0x06, 0, 1, 8, 0, 6, 4]
    ns = np.zeros(96, np.uint8)
    ns[12:14], ns[20], ns[54] = [0x86, 0xDD], 58, 135
    frames = [arp, arp, ns, ns, arp]
    lens = [64, 13, 78, 77, 19]       # a 13-byte frame whose stale bytes spell an ARP header
    pool = ingress.make_pool(frames, lens, range(5), 5, 128)
    for mode in (ingress.REF, ingress.WINDOW, ingress.FULL):
        out, desc, ts, ctrl, info = ingress.gather_host(pool, 128, np.arange(5), mode)
        assert ctrl.tolist() == [0, 2] and int(info["n_ctrl"]) == 2 and int(info["first_ctrl"]) == 0
    # FULL with a cut: the counts cover all n, the list only the positions below `packed`
    out, desc, ts, ctrl, info = ingress.gather_host(pool, 128, np.arange(5), ingress.FULL, 80)
    assert int(info["packed"]) == 2 and ctrl.tolist() == [0] and int(info["n_ctrl"]) == 2


def test_empty_burst():
    pool, _ = small_pool()
    for mode in (ingress.REF, ingress.WINDOW, ingress.FULL):
        out, desc, ts, ctrl, info = ingress.gather_host(pool, 128, np.zeros(0, np.uint32), mode)
        assert out.size == desc.size == ts.size == ctrl.size == 0
        want = np.zeros(1, layout.INGRESS_INFO_DTYPE)[0]
        want["first_bad"] = want["first_ctrl"] = NONE
        assert info == want


def test_argument_rules():
    pool, _ = small_pool()
    for stride in (120, 96, 2064):     # not a multiple of 16; below 16 + 96; larger than the pool
        with pytest.raises(ValueError):
            ingress.gather_host(pool, stride, [0], ingress.REF)
    with pytest.raises(ValueError):
        ingress.gather_host(pool, 128, [0], 3)
