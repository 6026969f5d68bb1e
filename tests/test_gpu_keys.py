"""upe_gpu_parse_keys and upe_gpu_match_keys on the device against their numpy mirror
(upe_amd/keys.py, pinned to the reference by tests/test_keys.py), bit for bit: every size around a
wave, a workgroup and a ragged last tile; the gate matrix under two fills; every matcher the rule
compiler can choose or be told to choose, on the tables that sit on its thresholds; the dry run of
a compiled image beside a loaded table.  Every output buffer is poisoned before the call and
followed by a canary that must survive it."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import gates
import golden_io
from test_gpu_rule_tables import workload
from test_keys import table_keys
from upe_amd import gpu, keys, layout, synth
from upe_amd.layout import FLOW_KEY_DTYPE

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 256, 4096 + 37)
POISON, CANARY, GUARD = 0xA7, 0xC5, 256


class Out:
    """A device output buffer of nbytes, poisoned, with GUARD canary bytes behind it."""

    def __init__(self, w, nbytes):
        self.w, self.nbytes = w, nbytes
        self.ptr = w.malloc(nbytes + GUARD)
        img = np.full(nbytes + GUARD, POISON, np.uint8)
        img[nbytes:] = CANARY
        w.h2d(self.ptr, img)
        w.sync()

    def fetch(self):
        self.w.sync()
        img = np.empty(self.nbytes + GUARD, np.uint8)
        self.w.d2h(img, self.ptr)
        self.w.sync()
        assert (img[self.nbytes:] == CANARY).all(), "the canary behind the output was written"
        self.w.free(self.ptr)
        return img[:self.nbytes]


def dev_in(w, a):
    a = np.ascontiguousarray(a)
    p = w.malloc(max(a.nbytes, 16))
    if a.nbytes:
        w.h2d(p, a.view(np.uint8).ravel())
    w.sync()
    return p


def gpu_parse(w, frames, desc, want_rc=True):
    """(key bytes (n, 44), rc or None, the frames buffer after the call)."""
    n = len(desc)
    df, dd = dev_in(w, frames), dev_in(w, desc)
    ok, orc = Out(w, 44 * n), Out(w, 4 * n)
    w.parse_keys(df, dd, n, ok.ptr, orc.ptr if want_rc else None)
    kb, rcb = ok.fetch(), orc.fetch()
    after = np.empty(frames.nbytes, np.uint8)
    w.d2h(after, df)
    w.sync()
    w.free(df)
    w.free(dd)
    if not want_rc:
        assert (rcb == POISON).all(), "rc was not asked for"
    return kb.reshape(n, 44), rcb.view(np.int32) if want_rc else None, after


def key_bytes(k):
    """The records as bytes, padding zero (numpy leaves a structured array's gaps alone)."""
    out = np.zeros(len(k), FLOW_KEY_DTYPE)
    for f in FLOW_KEY_DTYPE.names:
        out[f] = k[f]
    return out.view(np.uint8).reshape(len(k), 44)


def gpu_match(w, kbytes, image=None):
    n = len(kbytes)
    dk = dev_in(w, kbytes)
    out = Out(w, 4 * n)
    w.match_keys(dk, n, out.ptr, image=image)
    got = out.fetch().view(np.int32).copy()
    w.free(dk)
    return got


def check_parse(w, frames, desc, what, want_rc=True):
    want, want_rc_v = keys.parse_keys(frames, desc)
    kb, rc, after = gpu_parse(w, frames, desc, want_rc)
    if want_rc:
        assert np.array_equal(rc, want_rc_v), (what, np.nonzero(rc != want_rc_v)[0][:8])
    bad = np.nonzero((kb != key_bytes(want)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(desc)} keys differ, first {int(bad[0])}"
    assert np.array_equal(after, np.ascontiguousarray(frames).view(np.uint8).ravel()), \
        f"{what}: the frames were written"
    return want, want_rc_v


@functools.lru_cache(maxsize=None)
def _matrix(fill):
    return gates.matrix(fill, "shuffled")[0]


# ---------------------------------------------------------------------------------------------
# parse_keys
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_parse_keys_sizes(gpu_worker_factory, n):
    wl = _matrix("parent")
    assert wl.n >= n
    with gpu_worker_factory(16) as w:
        check_parse(w, wl.frames, wl.desc[:n], f"n={n}")


@pytest.mark.parametrize("fill", ["parent", "random"])
def test_parse_keys_gate_matrix(gpu_worker_factory, fill):
    """Every truncation of every header shape; the two fills differ only at and past len, and the
    mirror's keys (the expected value under both) do not depend on them."""
    wl = _matrix(fill)
    with gpu_worker_factory(16) as w:
        want, rc = check_parse(w, wl.frames, wl.desc, f"matrix {fill}")
    other = _matrix("random" if fill == "parent" else "parent")
    assert np.array_equal(wl.desc, other.desc) and not np.array_equal(wl.frames, other.frames)
    assert (rc == 0).any() and (rc == -1).any() and {4, 6} <= set(want["ip_ver"].tolist())


def test_parse_keys_control_subset_and_null_rc(gpu_worker_factory):
    wl, _, sid, _ = gates.control_subset()
    with gpu_worker_factory(16) as w:
        want, rc = check_parse(w, wl.frames, wl.desc, "control")
        check_parse(w, wl.frames, wl.desc, "control, rc NULL", want_rc=False)
    ctrl = sid >= 0
    assert ctrl.any() and (rc[ctrl] == -1).all() and not key_bytes(want)[ctrl].any()


# ---------------------------------------------------------------------------------------------
# match_keys
# ---------------------------------------------------------------------------------------------

def _no_catchall(rs):
    wild = ~(rs["src_mask"].any(axis=1) | rs["dst_mask"].any(axis=1) | (rs["src_port"] != 0) |
             (rs["dst_port"] != 0) | (rs["protocol"] != 0))
    return rs[~wild]


MATCH_TABLES = {
    "config_b_8": lambda: golden_io.load("config_b_small")[0].rules_sorted,
    "rand_prefix_61": lambda: workload("rand_prefix_61")[0].rules_sorted,
    "rand_prefix_64": lambda: workload("rand_prefix_64")[0].rules_sorted,
    "rand_prefix_65": lambda: workload("rand_prefix_65")[0].rules_sorted,
    "rand_bits_300": lambda: workload("rand_bits_300")[0].rules_sorted,          # non-prefix masks
    "no_catchall_300": lambda: _no_catchall(workload("rand_prefix_300")[0].rules_sorted),
    "only_v6_100": lambda: workload("only_v6_100")[0].rules_sorted,              # an empty list
    "only_v4_100": lambda: workload("only_v4_100")[0].rules_sorted,
    "v4_catchall_first": lambda: workload("v4_catchall_first")[0].rules_sorted,
    "both_catchall_first": lambda: workload("both_catchall_first")[0].rules_sorted,
    # config D's shape (exact flows in few mask signatures), at the compiler's own threshold for a
    # tuple-space index (1024 rules)
    "config_d_1024": lambda: synth.config_d(n=64, n_rules=1024).rules_sorted,
}
MODES = ("default", "scan", "tree", "tss")


@functools.lru_cache(maxsize=None)
def _table(name):
    rs = MATCH_TABLES[name]()
    k = table_keys(rs, 23, 1500)
    clean = key_bytes(k)
    # the same keys with everything that is not part of a key set: all padding, and an IPv4
    # key's union bytes 4-15
    dirty = clean.copy()
    dirty[:, 1:4] = 0xFF
    dirty[:, 41:44] = 0xFF
    v4 = k["ip_ver"] == 4
    dirty[v4, 8:20] = 0xFF
    dirty[v4, 24:36] = 0xFF
    want = keys.match_keys(rs, k)
    assert v4.any() and (k["ip_ver"] == 6).any() and want[:3].tolist() == [-1, -1, -1]
    return rs, np.concatenate([clean, dirty]), np.concatenate([want, want])


def _set_mode(monkeypatch, mode):
    for k in ("UPE_GPU_TSS", "UPE_GPU_TREE", "UPE_GPU_TREE_LDS", "UPE_GPU_FP_STAGE",
              "UPE_GPU_TREE_BINTH"):
        monkeypatch.delenv(k, raising=False)
    if mode != "default":
        monkeypatch.setenv("UPE_GPU_TSS", "1" if mode == "tss" else "0")
        monkeypatch.setenv("UPE_GPU_TREE", "0" if mode == "scan" else "1")


def _want_kind(mode, name, nrules):
    if mode == "tss":
        return 1
    if mode == "scan":
        return 0
    if mode == "tree":
        return 2 if nrules >= 61 else 0   # pad = (ceil(count / 4) + 1) * 4 > 64
    return 1 if name == "config_d_1024" else None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(MATCH_TABLES))
def test_match_keys_tables(gpu_worker_factory, monkeypatch, name, mode):
    rs, kb, want = _table(name)
    _set_mode(monkeypatch, mode)
    with gpu_worker_factory(1024) as w:
        w.load_rules(rs)
        kind = w.rule_index_kind()
        wk = _want_kind(mode, name, len(rs))
        assert wk is None or kind == wk, f"{name} {mode}: index kind {kind}, wanted {wk}"
        got = gpu_match(w, kb)
        # the same through a compiled image beside the loaded table
        image = gpu.RuleImage(rs, 1024)
        got_dry = gpu_match(w, kb, image=image)
        image.free()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (f"{name} {mode} (kind {kind}): {bad.size} of {len(want)} keys differ, "
                           f"first {int(bad[0])}: {int(got[bad[0]])} vs {int(want[bad[0]])}")
    assert np.array_equal(got_dry, want), f"{name} {mode}: the dry run differs"
    assert (want >= 0).any() and (want == -1).any()


@pytest.mark.parametrize("n", SIZES)
def test_match_keys_sizes(gpu_worker_factory, monkeypatch, n):
    _set_mode(monkeypatch, "default")
    rs, kb, want = _table("rand_prefix_65")
    reps = -(-max(n, 1) // len(kb))
    kb, want = np.tile(kb, (reps, 1))[:n], np.tile(want, reps)[:n]
    with gpu_worker_factory(1024) as w:
        w.load_rules(rs)
        assert np.array_equal(gpu_match(w, kb), want)


def _state(w):
    c, s = w.get_stats()
    return c.tobytes(), s.tobytes(), w.get_l1().tobytes(), w.launch_info()


def test_dry_run_leaves_the_context_alone(gpu_worker_factory, monkeypatch):
    _set_mode(monkeypatch, "default")
    wl = golden_io.load("config_c_small")[0]
    rs_a = wl.rules_sorted
    rs_b, kb, want_b = _table("rand_bits_300")
    want_a = keys.match_keys(rs_a, kb.copy().view(FLOW_KEY_DTYPE).ravel())
    assert not np.array_equal(want_a, want_b)
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.run()
        _, v0 = b.fetch()
        b.free()
        before = _state(w)
        image = gpu.RuleImage(rs_b, 1024)
        for _ in range(2):   # the image is not consumed
            assert np.array_equal(gpu_match(w, kb, image=image), want_b)
        assert np.array_equal(gpu_match(w, kb), want_a), "the loaded table is still A"
        assert _state(w) == before
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.run()
        _, v1 = b.fetch()
        b.free()
        assert np.array_equal(layout.verdict_rule(v1), layout.verdict_rule(v0))
        assert np.array_equal(layout.verdict_code(v1), layout.verdict_code(v0))
        assert np.array_equal(layout.verdict_rule(v0), keys.match_keys(
            rs_a, keys.parse_keys(wl.frames, wl.desc)[0]))
        # and the image still reloads
        w.reload_image(image)
        assert np.array_equal(gpu_match(w, kb), want_b)
        image.free()


@pytest.mark.parametrize("case", ["config_c_small", "config_d_small"])
def test_composition_on_the_device(gpu_worker_factory, monkeypatch, case):
    _set_mode(monkeypatch, "default")
    wl = golden_io.load(case)[0]
    n = wl.n
    with gpu_worker_factory(wl.capacity) as w:
        w.configure(wl)
        df, dd = dev_in(w, wl.frames), dev_in(w, wl.desc)
        dk, out = Out(w, 44 * n), Out(w, 4 * n)
        w.parse_keys(df, dd, n, dk.ptr, None)
        w.match_keys(dk.ptr, n, out.ptr)
        got = out.fetch().view(np.int32)
        dk.fetch()
        w.free(df)
        w.free(dd)
        b = gpu.DeviceBatch(w, wl.frames, wl.desc)
        b.run()
        _, verdict = b.fetch()
        b.free()
    assert np.array_equal(got, layout.verdict_rule(verdict))
    assert (got >= 0).any() and (got == -1).any()


def test_argument_errors_launch_nothing(gpu_worker_factory):
    L = gpu.LIB
    rs = golden_io.load("config_b_small")[0].rules_sorted
    with gpu_worker_factory(16) as w:
        c = w._ctx
        buf = w.malloc(4096)
        before = w.launch_info()
        assert L.upe_gpu_parse_keys(None, buf, buf, 1, buf, None, None) == -1
        assert b"null context" in L.upe_gpu_last_error()
        assert L.upe_gpu_match_keys(None, None, buf, 1, buf, None) == -1
        assert b"null context" in L.upe_gpu_last_error()
        for args in ((c, None, buf, 1, buf, None, None), (c, buf, None, 1, buf, None, None),
                     (c, buf, buf, 1, None, None, None)):
            assert L.upe_gpu_parse_keys(*args) == -1
            assert b"null buffer" in L.upe_gpu_last_error()
        assert L.upe_gpu_parse_keys(c, buf, buf, 1 << 32, buf, None, None) == -1
        assert b"32 bits" in L.upe_gpu_last_error()
        # no rules loaded since the context was opened
        assert L.upe_gpu_match_keys(c, None, buf, 1, buf, None) == -1
        assert b"no rule table" in L.upe_gpu_last_error()
        w.load_rules(rs)
        for args in ((c, None, None, 1, buf, None), (c, None, buf, 1, None, None)):
            assert L.upe_gpu_match_keys(*args) == -1
            assert b"null buffer" in L.upe_gpu_last_error()
        assert L.upe_gpu_match_keys(c, None, buf, 1 << 32, buf, None) == -1
        assert b"32 bits" in L.upe_gpu_last_error()
        # n == 0 is a no-op, whatever the buffers
        assert L.upe_gpu_parse_keys(c, None, None, 0, None, None, None) == 0
        assert L.upe_gpu_match_keys(c, None, None, 0, None, None) == 0
        assert w.launch_info() == before
        w.free(buf)
