"""The egress batch on the host: egress.pack_host (the numpy restatement of upe_gpu_egress_pack's
packing rule, include/upe_gpu.h) against the reference's own forwarded frames, and
upe_tx_flush_packed (the reference worker's TX calls from the packed batch, src/worker.c:287-303)
against upe_tx_flush over the classified ingress batch and, where oracle/_ref is built, against
the log of src/worker.c's own tx_send_batch calls.  No GPU: the verdicts and rewritten frames are
the golden (reference) ones; the device side is tests/test_gpu_egress_pack.py."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import golden_io
import oracle
from upe_amd import egress, gpu
from upe_amd.layout import V_FWD, desc_lens, desc_offsets

CASES = ["config_a", "config_b_small", "config_c_small", "config_cf_small", "config_d_small"]
WORKER_BURST_SIZE = 32   # reference include/worker.h


def slotted_records(frames_in, frames_out, desc, verdict) -> np.ndarray:
    """The emit-mode records of a batch as the device lays them out (UPE_HDR_SLOT: a cursor over
    the forwarded packets, reset at every multiple of 64), built from the reference's output
    frames; the slots no forwarded packet owns hold garbage."""
    offs = desc_offsets(desc)
    rec = np.full((len(offs), 16), 0xEE, np.uint8)
    cursor = 0
    for i in range(len(offs)):
        if i % 64 == 0:
            cursor = i
        if (int(verdict[i]) & 0xF) != V_FWD:
            continue
        o = int(offs[i])
        got = frames_out[o:o + 26]
        r = rec[cursor]
        cursor += 1
        r[:12] = got[:12]
        if frames_in[o + 12] == 0x86 and frames_in[o + 13] == 0xDD:
            r[12], r[13], r[14], r[15] = got[21], 0, 0, 6
        else:
            r[12], r[13], r[14], r[15] = got[22], got[24], got[25], 4
    return rec


@functools.lru_cache(maxsize=None)
def _packed(case):
    wl, ref = golden_io.load(case)
    return wl, ref, egress.pack_host(ref["frames"], wl.desc, ref["verdict"])


@pytest.mark.parametrize("case", CASES)
def test_pack_host_gives_the_reference_frames(case):
    wl, ref, (out, out_desc, out_index, info) = _packed(case)
    fwd = np.nonzero((ref["verdict"] & 0xF) == V_FWD)[0]
    assert fwd.size > 0 or case == "config_a"   # config A forwards nothing: an empty batch
    assert np.array_equal(out_index, fwd)
    assert int(info["frames"]) == int(info["packed"]) == fwd.size == len(out_desc)
    assert int(info["bytes"]) == int(info["need"]) == out.size
    offs, lens = desc_offsets(wl.desc), desc_lens(wl.desc)
    po, pl = desc_offsets(out_desc), desc_lens(out_desc)
    at = 0
    for k, i in enumerate(fwd):
        assert po[k] == at and at % 16 == 0, f"frame {k} at {po[k]}, expected {at}"
        assert pl[k] == lens[i]
        want = ref["frames"][offs[i]:offs[i] + lens[i]]
        assert np.array_equal(out[at:at + lens[i]], want), f"frame {k} (packet {i}) differs"
        end = at + ((int(lens[i]) + 15) & ~15)
        assert not out[at + lens[i]:end].any(), f"pad after frame {k} is not zero"
        at = end
    assert at == out.size


@pytest.mark.parametrize("case", CASES)
def test_pack_host_hdr_mode_is_byte_identical(case):
    """The untouched ingress frames plus the records in the UPE_HDR_SLOT layout give the bytes of
    the in-place mode; and the same through the library's own upe_hdr_apply."""
    wl, ref, (out, out_desc, out_index, info) = _packed(case)
    rec = slotted_records(wl.frames, ref["frames"], wl.desc, ref["verdict"])
    got = egress.pack_host(wl.frames, wl.desc, ref["verdict"], hdr=rec)
    assert np.array_equal(got[0], out)
    assert np.array_equal(got[1], out_desc) and np.array_equal(got[2], out_index)
    assert got[3] == info
    applied = gpu.hdr_apply(wl.frames, wl.desc, gpu.expand_records(rec, ref["verdict"]))
    assert np.array_equal(egress.pack_host(applied, wl.desc, ref["verdict"])[0], out)


def test_pack_host_patch_stops_at_len():
    """A patched byte position at or beyond len is not written: frames of 10, 22 and 25 bytes."""
    lens = np.array([10, 22, 25, 60])
    frames = np.arange(4 * 64, dtype=np.uint8) | 1
    desc = (np.arange(4, dtype=np.uint64) * 64 << np.uint64(16)) | lens.astype(np.uint64)
    verdict = np.full(4, V_FWD, np.uint32)
    rec = np.zeros((4, 16), np.uint8)
    rec[:, 15] = [4, 4, 4, 6]
    out, out_desc, _, info = egress.pack_host(frames, desc, verdict, hdr=rec)
    assert int(info["bytes"]) == 16 + 32 + 32 + 64
    po = desc_offsets(out_desc)
    for k, ln in enumerate(lens):
        want = frames[64 * k:64 * k + ln].copy()
        want[:min(12, ln)] = 0
        for pos in ((22, 24, 25) if k < 3 else (21,)):
            if pos < ln:
                want[pos] = 0
        assert np.array_equal(out[po[k]:po[k] + ln], want), k
        assert not out[po[k] + ln:po[k] + ((ln + 15) & ~15)].any()


def test_pack_host_capacity():
    wl, ref, (out, out_desc, out_index, info) = _packed("config_c_small")
    need = int(info["need"])
    ends = desc_offsets(out_desc) + ((desc_lens(out_desc) + 15) & ~15)
    for cap, packed in ((0, 0), (int(ends[0]) - 1, 0), (int(ends[0]), 1), (int(ends[6]) + 15, 7),
                        (need - 1, len(ends) - 1), (need, len(ends)), (need + 100, len(ends))):
        o, d, x, inf = egress.pack_host(ref["frames"], wl.desc, ref["verdict"], out_bytes=cap)
        used = int(ends[packed - 1]) if packed else 0
        assert (int(inf["frames"]), int(inf["packed"]), int(inf["bytes"]), int(inf["need"])) == \
            (len(ends), packed, used, need), cap
        assert np.array_equal(o, out[:used]) and np.array_equal(d, out_desc[:packed])
        assert np.array_equal(x, out_index[:packed])


def _same_calls(got, want):
    assert [b[0].tolist() for b in got[0]] == [b[0].tolist() for b in want[0]], "TX calls differ"
    assert [b[1] for b in got[0]] == [b[1] for b in want[0]], "TX frame bytes differ"
    assert got[1:] == want[1:], "forwarded / dropped differ"


@pytest.mark.parametrize("burst", [1, 7, 32, 64])
@pytest.mark.parametrize("case", CASES)
def test_tx_flush_packed_equals_tx_flush(case, burst):
    wl, ref, (out, out_desc, out_index, _) = _packed(case)
    want = gpu.tx_flush(ref["frames"], wl.desc, ref["verdict"], burst)
    got = gpu.tx_flush_packed(out, out_desc, out_index, burst)
    assert want[1] == len(out_index) and want[2] == 0
    _same_calls(got, want)
    if burst == WORKER_BURST_SIZE and oracle.ref_available():
        oracle.run_reference(wl)
        sizes, order = oracle.tx_log()
        assert [len(b[0]) for b in got[0]] == sizes.tolist(), "TX call sizes differ"
        sent = [b[0] for b in got[0]] + [np.zeros(0, np.int64)]
        assert np.array_equal(np.concatenate(sent), order.astype(np.int64)), "TX order differs"


@pytest.mark.parametrize("sent_of", [lambda c: c // 2, lambda c: -1, lambda c: c + 5],
                         ids=["half", "failing", "too_many"])
def test_tx_flush_packed_partial_sends(sent_of):
    """sendmmsg sending fewer than asked, or failing: forwarded += sent, dropped += count - sent
    (src/worker.c:288-294), as upe_tx_flush counts them."""
    wl, ref, (out, out_desc, out_index, _) = _packed("config_b_small")
    want = gpu.tx_flush(ref["frames"], wl.desc, ref["verdict"], WORKER_BURST_SIZE, sent_of=sent_of)
    got = gpu.tx_flush_packed(out, out_desc, out_index, WORKER_BURST_SIZE, sent_of=sent_of)
    _same_calls(got, want)
    assert got[1] + got[2] == len(out_index)


def _refused(out, out_desc, out_index, burst, match):
    calls = []
    with pytest.raises(gpu.UpeGpuError, match=match):
        gpu.tx_flush_packed(out, out_desc, out_index, burst,
                            sent_of=lambda c: calls.append(c) or c)
    assert calls == [], "a send was made before the refusal"


@pytest.mark.parametrize("burst", [0, 65])
def test_tx_flush_packed_burst_out_of_range(burst):
    _, _, (out, out_desc, out_index, _) = _packed("config_b_small")
    _refused(out, out_desc, out_index, burst, "burst")


@pytest.mark.parametrize("how", ["repeated", "descending"])
def test_tx_flush_packed_refuses_a_list_out_of_order(how):
    """All or nothing: the bad entry sits near the end, and still no send is made."""
    _, _, (out, out_desc, out_index, _) = _packed("config_b_small")
    bad = out_index.copy()
    k = len(bad) - 3
    bad[k] = bad[k - 1] if how == "repeated" else bad[k - 1] - 1
    _refused(out, out_desc, bad, WORKER_BURST_SIZE, "ascend")


def test_tx_flush_packed_empty():
    got = gpu.tx_flush_packed(np.zeros(0, np.uint8), np.zeros(0, np.uint64),
                              np.zeros(0, np.uint32), 32)
    assert got == ([], 0, 0)
