"""The release order on the host: release.order_host (numpy), upe_release_order_host (C) and
upe_release_flush against a plain sequential restatement of the reference's worker_main, over
tests/release_cases.py.  No GPU."""
from __future__ import annotations

import os
import subprocess
import tempfile

import numpy as np
import pytest

import release_cases as rc
from upe_amd import gpu, release
from upe_amd.layout import V_CONSUMED, V_FWD, VF_ARP_REPLY, make_desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = gpu.RELEASE_POISON


def worker_main(verdict, bursts, handle_of=lambda i: i):
    """What the reference's worker_main does with each buffer, per burst, as the verdict words tell
    it: [(tx_send positions, frees in order, tx_send_batch positions)], from a loop that follows
    src/worker.c line by line."""
    out = []
    for s, e in bursts:                              # src/worker.c:268 ring_pop_burst
        sends, frees, tx_bufs = [], [], []           # tx_count = 0 (src/worker.c:302)
        for i in range(s, e):                        # src/worker.c:282-284 process_packet
            w = int(verdict[i])
            if w & VF_ARP_REPLY:
                sends.append(i)                      # src/worker.c:51 tx_send, before any free
            if (w & 0xF) == V_FWD:
                tx_bufs.append(i)                    # src/worker.c:240-243 queued, not freed
            else:
                frees.append(handle_of(i))           # src/worker.c:97, 123, 135, 151, 170, 209, 252
        if tx_bufs:                                  # src/worker.c:287
            frees += [handle_of(i) for i in tx_bufs]   # src/worker.c:296-301, after :288
        out.append((sends, frees, tx_bufs))
    return out


def check_twin(case, got, slot=None, what=""):
    """(order, handle, burst_fwd, reply, info) over a poison, with room behind: against the
    restatement and the numpy form, bit for bit."""
    order, handle, bf, reply, info = got
    n, bursts = case.n, case.bursts
    want = worker_main(case.verdict, bursts)
    exp = release.order_host(case.verdict, slot=slot, **case.form)
    flat = [i for _, frees, _ in want for i in frees]
    assert order[:n].tolist() == flat == exp.order.tolist(), what
    assert bf[:len(bursts)].tolist() == [len(t) for _, _, t in want] == exp.burst_fwd.tolist(), what
    sends = [i for s, _, _ in want for i in s]
    assert reply[:len(sends)].tolist() == sends == exp.reply.tolist(), what
    for (s, e), (_, frees, tx) in zip(bursts, want):
        assert order[e - len(tx):e].tolist() == tx, what     # the tx_send_batch argument list
    if slot is not None:
        assert handle[:n].tolist() == slot[order[:n]].tolist() == exp.handle.tolist(), what
        assert (handle[n:] == P).all(), what
    assert (order[n:] == P).all() and (bf[len(bursts):] == P).all(), what
    assert (reply[len(sends):] == P).all(), what
    assert info.tobytes() == exp.info.tobytes(), (what, info, exp.info)
    code = case.verdict & 0xF
    assert int(info["forwarded"]) == int((code == V_FWD).sum())
    assert int(info["consumed"]) == int((code == V_CONSUMED).sum())
    assert int(info["dropped"]) == n - int(info["forwarded"]) - int(info["consumed"])
    assert int(info["first_reply"]) == (sends[0] if sends else 2**64 - 1)
    # the forwarded ranges concatenated are the batch's forwarded packets in order
    fwd = np.concatenate([order[e - int(bf[b]):e] for b, (s, e) in enumerate(bursts)])
    assert fwd.tolist() == np.nonzero(code == V_FWD)[0].tolist(), what


@pytest.mark.parametrize("n", rc.SIZES)
def test_twins_follow_worker_main(n):
    for k, case in enumerate(rc.cases(n)):
        slot = rc.slots(n, ("permuted", "repeat", "descend")[k % 3]) if k % 2 else None
        check_twin(case, gpu.release_order_host(case.verdict, slot=slot, **case.form), slot,
                   case.name)


def frames_for(n):
    """Frames the flush can point into: packet i is 16 + i % 48 bytes at 64 i."""
    frames = (np.arange(64 * n + 96) % 251).astype(np.uint8)
    return frames, make_desc(64 * np.arange(n), 16 + np.arange(n) % 48)


def split_events(events, bursts):
    """The flush's events cut into bursts by the buffers released: [(send_one positions, frees,
    tx_send_batch positions or [])], checking each burst's shape on the way: replies, the frees of
    the packets not forwarded, the batch, the frees of its buffers."""
    out, k = [], 0
    for s, e in bursts:
        sends, frees, tx, stage = [], [], [], 0
        while len(frees) < e - s:
            ev = events[k]
            k += 1
            if ev[0] == "send_one":
                assert stage == 0, "a reply after a free of its burst"
                sends.append(ev[1])
            elif ev[0] == "release":
                assert stage in (0, 2) and ev[1], "an empty or misplaced release"
                frees += ev[1]
                stage = 1 if stage == 0 else 3
            else:
                assert stage in (0, 1), "a second batch in one burst"
                tx = ev[1].tolist()
                stage = 2
        assert stage in (1, 3) and len(frees) == e - s
        out.append((sends, frees, tx))
    assert k == len(events), "events after the last burst"
    return out


@pytest.mark.parametrize("n", (1, 65, 257, 1025, 4 * 1024 + 37))
def test_flush_makes_worker_mains_calls(n):
    frames, desc = frames_for(n)
    offs, lens = (desc >> np.uint64(16)).astype(int), (desc & np.uint64(0xFFFF)).astype(int)
    for k, case in enumerate(rc.cases(n)):
        slot = rc.slots(n, "permuted") if k % 2 else None
        r = release.order_host(case.verdict, slot=slot, **case.form)
        short = (lambda c: c - 1) if k % 3 == 0 else None    # sendmmsg reports one frame fewer
        events, fwd, drp = gpu.release_flush(frames, desc, r.order, r.burst_fwd, handle=r.handle,
                                             reply=r.reply, sent_of=short, **case.form)
        got = split_events(events, case.bursts)
        want = worker_main(case.verdict, case.bursts,
                           (lambda i: i) if slot is None else (lambda i: int(slot[i])))
        # the regrouping: per burst the same sends, the same frees, the same batch; over the batch
        # therefore the same sequence of frees and the same sequence of sends
        assert got == want, case.name
        for ev in events:
            if ev[0] == "send_one":
                i = ev[1]
                assert ev[2] == bytes(frames[offs[i]:offs[i] + lens[i]]), case.name
        if slot is None:   # handles are positions: a reply goes out before its own buffer is freed
            seen = set()
            for ev in events:
                if ev[0] == "release":
                    seen.update(ev[1])
                elif ev[0] == "send_one":
                    assert ev[1] not in seen, case.name
        # the batches and the accounting are upe_tx_flush's on the same verdicts and bursts
        if case.burst:
            batches, f2, d2 = gpu.tx_flush(frames, desc, case.verdict, burst=case.burst,
                                           sent_of=short)
            mine = [ev for ev in events if ev[0] == "send"]
            assert len(mine) == len(batches) and (fwd, drp) == (f2, d2), case.name
            for ev, (idx, data) in zip(mine, batches):
                assert ev[1].tolist() == idx.tolist() and ev[2] == data, case.name
        total = int(r.info["forwarded"])
        calls = sum(1 for ev in events if ev[0] == "send")
        assert fwd + drp == total and (drp == calls if short else drp == 0), case.name


@pytest.mark.parametrize("n", (130, 1024, 2049))
def test_bad_burst_arrays_touch_nothing_else(n):
    v = rc.with_replies(rc.words(rc.fwd_mask(n, 3)), rc.SHAPES["64s"](n), "every_burst")
    good = release.order_host(v, burst=64)
    for name, (first, count) in rc.bad_arrays(n).items():
        assert release.bad_bursts(first, n) == count, name
        exp = release.order_host(v, first=first)
        assert exp.order is None and int(exp.info["bad_bursts"]) == count, name
        order, handle, bf, reply, info = gpu.release_order_host(v, first=first,
                                                                slot=rc.slots(n, "repeat"))
        for a in (order, handle, bf, reply):
            assert (a == P).all(), name
        assert info.tobytes() == exp.info.tobytes(), name
        for f in ("forwarded", "consumed", "dropped", "replies", "first_reply"):
            assert info[f] == good.info[f], (name, f)
        assert int(info["bursts"]) == len(first) - 1


def refused_order(n=100):
    """name -> arguments upe_release_order_host (and the device call) refuse."""
    v = rc.words(rc.fwd_mask(n))
    first = rc.SHAPES["cycle"](n)
    return {
        "burst_0": dict(verdict=v, burst=0),
        "burst_65": dict(verdict=v, burst=65),
        "nb_0": dict(verdict=v, first=first, nb=0),
        "nb_above_n": dict(verdict=v[:3], first=np.array([0, 1, 2, 3, 3], np.uint32), nb=4),
    }


def test_refused_arguments_order_host():
    for name, kw in refused_order().items():
        with pytest.raises(gpu.UpeGpuError):
            gpu.release_order_host(**kw)
    v = rc.words(rc.fwd_mask(10))
    buf = np.full(32, P, np.uint32)
    info = np.zeros(1, gpu.RELEASE_INFO_DTYPE)
    p = gpu._np_ptr
    call = gpu.LIB.upe_release_order_host
    # no info; no verdicts, order or burst counts with n > 0; one of slot / handle
    assert call(p(v), 10, None, 0, 4, None, p(buf), None, p(buf), None, None) == -1
    assert call(None, 10, None, 0, 4, None, p(buf), None, p(buf), None, p(info)) == -1
    assert call(p(v), 10, None, 0, 4, None, None, None, p(buf), None, p(info)) == -1
    assert call(p(v), 10, None, 0, 4, None, p(buf), None, None, None, p(info)) == -1
    assert call(p(v), 10, None, 0, 4, p(v), p(buf), None, p(buf), None, p(info)) == -1
    assert call(p(v), 10, None, 0, 4, None, p(buf), p(buf), p(buf), None, p(info)) == -1
    assert call(p(v), 2**32 - 1024, None, 0, 4, None, p(buf), None, p(buf), None, p(info)) == -1
    assert (buf == P).all() and not info.view(np.uint8).any()
    # n == 0: info alone, zero but for first_reply
    assert call(None, 0, None, 0, 4, None, None, None, None, None, p(info)) == 0
    assert info.view(np.uint64).tolist() == [0, 0, 0, 0, 0, 0, 2**64 - 1, 0]


def test_refused_arguments_flush():
    n = 200
    frames, desc = frames_for(n)
    first = rc.SHAPES["cycle"](n)
    v = rc.with_replies(rc.words(rc.fwd_mask(n, 5)), first, "every_burst")
    r = release.order_host(v, first=first)
    ok = dict(order=r.order, burst_fwd=r.burst_fwd, first=first, reply=r.reply)
    events, _, _ = gpu.release_flush(frames, desc, **ok)
    assert events

    def change(key, at, value):
        a = ok[key].copy()
        a[at] = value
        return {**ok, key: a}

    bad = {
        "burst_0": {**ok, "first": None, "burst": 0},
        "burst_65": {**ok, "first": None, "burst": 65},
        "nb_0": {**ok, "nb": 0},
        "nb_above_n": {**ok, "nb": n + 1, "first": np.arange(n + 2, dtype=np.uint32)},
        "fwd_above_size": change("burst_fwd", 2, 4),            # burst 2 holds three packets
        "order_outside": change("order", 3, 2),                 # entry 3 belongs to [3, 6)
        "order_past": change("order", 3, 6),
        "reply_equal": change("reply", 1, int(r.reply[0])),
        "reply_descends": {**ok, "reply": r.reply[::-1].copy()},
        "reply_past_n": change("reply", -1, n),
    }
    for name, (f, _) in rc.bad_arrays(n).items():
        bad["first:" + name] = {**ok, "first": f}
    for name, kw in bad.items():
        calls = []
        with pytest.raises(gpu.UpeGpuError):
            gpu.release_flush(frames, desc, sent_of=lambda c: calls.append(c) or c, **kw)
        # release_flush's own callbacks append to a list it only returns: count through ctypes
        assert not calls, name
    # no callback at all: the three of them counted
    made = []
    ops = gpu.ReleaseOps(gpu.TX_SEND_FN(lambda u, f, ln: made.append(1) or 0),
                         gpu.TX_BATCH_FN(lambda u, f, ln, c: made.append(1) or c),
                         gpu.RELEASE_FN(lambda u, h, c: made.append(1)))
    import ctypes
    p = gpu._np_ptr
    for name, kw in bad.items():
        f = kw.get("first")
        nb = kw.get("nb", 0 if f is None else len(f) - 1)
        rcode = gpu.LIB.upe_release_flush(p(frames), p(desc), p(kw["order"]), None,
                                          None if f is None else p(f), nb, kw.get("burst", 0), n,
                                          p(kw["burst_fwd"]), p(kw["reply"]), len(kw["reply"]),
                                          ctypes.byref(ops), None, None, None)
        assert rcode == -1 and not made, name
    # null arguments
    args = [p(frames), p(desc), p(r.order), None, p(first), len(first) - 1, 0, n, p(r.burst_fwd),
            p(r.reply), len(r.reply), ctypes.byref(ops), None, None, None]
    for at in (0, 1, 2, 8, 9, 11):
        a = list(args)
        a[at] = None
        assert gpu.LIB.upe_release_flush(*a) == -1 and not made, at
    none = gpu.ReleaseOps()
    a = list(args)
    a[11] = ctypes.byref(none)
    assert gpu.LIB.upe_release_flush(*a) == -1


def test_release_san_runs_clean():
    """`make release-san`: the two host functions under ASan and UBSan in a stand-alone program
    (tools/release_san.c), against a sequential loop written out there."""
    with tempfile.TemporaryDirectory() as d:
        out = subprocess.run(["make", "-C", os.path.join(ROOT, "upe_amd", "csrc"), "release-san",
                              f"BUILD={d}/"], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "release_san: OK" in out.stdout
