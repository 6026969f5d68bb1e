"""The host mirror of the flow-key calls (upe_amd/keys.py) against the restated reference, so that
the device comparison of tests/test_gpu_keys.py cannot pass on a wrong yardstick: parse_keys
against upe_ref_parse (all 44 bytes and rc), match_keys against upe_rules_match_host and the
restated match_rule loop, and their composition against the worker's verdicts.  No GPU."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import gates
import golden_io
import oracle
from test_gpu_rule_tables import workload
from test_rule_index import boundary_keys, random_table, ref_match
from upe_amd import gpu, keys, layout
from upe_amd.layout import FLOW_KEY_DTYPE

PARSE_CASES = ("matrix", "boundary", "edge_zero", "edge_consistent", "edge_inconsistent",
               "config_d_small")
GOLDEN_SMALL = ("config_b_small", "config_c_small", "config_d_small")
ADVERSARIAL = ("rand_prefix_61", "rand_bits_61", "rand_bits_300", "only_v6_100", "only_v4_100",
               "v4_catchall_first", "both_catchall_first", "dups_ties_200")


@functools.lru_cache(maxsize=None)
def _batch(case):
    if case == "matrix":
        return gates.matrix("parent")[0]
    if case == "boundary":
        return gates.boundary_subset()[0]
    return golden_io.load(case)[0]


def oracle_keys(wl):
    """upe_ref_parse per packet: (keys, rc); a failed parse's key is zeroed, as the calls do."""
    offs, lens = layout.desc_offsets(wl.desc), layout.desc_lens(wl.desc)
    out = np.zeros(wl.n, FLOW_KEY_DTYPE)
    rc = np.zeros(wl.n, np.int32)
    raw = out.view(np.uint8).reshape(wl.n, 44)
    for i in range(wl.n):
        o, ln = int(offs[i]), int(lens[i])
        rc[i], k = oracle.parse(bytes(wl.frames[o:o + min(ln, 128)]), ln)
        if rc[i] == 0:
            raw[i] = k
    return out, rc


@pytest.mark.parametrize("case", PARSE_CASES)
def test_parse_keys_equals_the_reference_parser(case):
    wl = _batch(case)
    want, want_rc = oracle_keys(wl)
    got, rc = keys.parse_keys(wl.frames, wl.desc)
    assert rc.dtype == np.int32 and got.dtype == FLOW_KEY_DTYPE
    assert np.array_equal(rc, want_rc), np.nonzero(rc != want_rc)[0][:8]
    g, w = got.view(np.uint8).reshape(-1, 44), want.view(np.uint8).reshape(-1, 44)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, f"{case}: {bad.size} keys differ, first {int(bad[0])}"
    assert not g[rc != 0].any(), "a failed parse leaves 44 zero bytes"
    # not hollow: both outcomes, and for the matrix both families
    assert (rc == 0).any() and (rc != 0).any()
    if case in ("matrix", "boundary", "config_d_small"):
        assert {4, 6} <= set(got["ip_ver"].tolist())


def test_parse_keys_ignores_bytes_past_len():
    """The same frames over two fills: the keys must not move."""
    a = gates.boundary_subset("parent")[0]
    b = gates.boundary_subset("random")[0]
    assert np.array_equal(a.desc, b.desc) and not np.array_equal(a.frames, b.frames)
    ka, ra = keys.parse_keys(a.frames, a.desc)
    kb, rb = keys.parse_keys(b.frames, b.desc)
    assert ka.tobytes() == kb.tobytes() and np.array_equal(ra, rb)


def test_parse_keys_control_frames_fail():
    wl, _, sid, _ = gates.control_subset()
    got, rc = keys.parse_keys(wl.frames, wl.desc)
    ctrl = sid >= 0
    assert ctrl.any() and (rc[ctrl] == -1).all()
    assert not got.view(np.uint8).reshape(-1, 44)[ctrl].any()
    assert (rc[~ctrl] == 0).all()


def _tables():
    out = {c: golden_io.load(c)[0].rules_sorted for c in ("config_b_small", "config_c_small")}
    out.update({t: workload(t)[0].rules_sorted for t in ADVERSARIAL})
    rng = np.random.default_rng(41)
    out["rand_no_prefix_120"] = random_table(rng, 120, False)
    return out


def table_keys(rs, seed, n=1500):
    """boundary_keys of the table, an eighth moved to the other family, and three foreign
    versions."""
    rng = np.random.default_rng(seed)
    k = boundary_keys(rs, rng, n)
    other = rng.random(n) < 0.125
    k["ip_ver"] = np.where(other, 10 - k["ip_ver"], k["ip_ver"])
    k["ip_ver"][:3] = (0, 5, 255)
    return k


@pytest.mark.parametrize("name", list(_tables()))
def test_match_keys_equals_host_matcher_and_reference(name):
    rs = _tables()[name]
    k = table_keys(rs, 7)
    got = keys.match_keys(rs, k)
    host, _ = gpu.rules_match_host(rs, k)
    assert got.dtype == np.int32
    assert np.array_equal(got, host), np.nonzero(got != host)[0][:8]
    assert got[:3].tolist() == [-1, -1, -1]
    # the restated match_rule loop, for the versions the reference's parser can produce
    fam = (k["ip_ver"] == 4) | (k["ip_ver"] == 6)
    assert np.array_equal(got[fam], ref_match(rs, k[fam]))
    assert {4, 6} <= set(k["ip_ver"].tolist())


def test_match_keys_coverage_first_last_none():
    """The key sets reach the first rule, the last rule and no rule, in both families: a
    degenerate batch fails here."""
    rs = workload("rand_prefix_61")[0].rules_sorted
    wild = ~(rs["src_mask"].any(axis=1) | rs["dst_mask"].any(axis=1) | (rs["src_port"] != 0) |
             (rs["dst_port"] != 0) | (rs["protocol"] != 0))
    rs = rs[~wild]   # no catch-all: either family can come away with nothing
    k = table_keys(rs, 7, 4000)
    # each rule's own value, so that the first and the last rule are asked for by name
    own = np.zeros(len(rs), FLOW_KEY_DTYPE)
    for f in ("src_ip", "dst_ip", "src_port", "dst_port", "protocol"):
        own[f] = rs[f]
    own["src_ip"] &= rs["src_mask"]
    own["dst_ip"] &= rs["dst_mask"]
    own["ip_ver"] = np.where(rs["ip_ver"] == 0, 4, rs["ip_ver"])
    k = np.concatenate([k, own])
    got = keys.match_keys(rs, k)
    assert (got == 0).any() and (got == -1).any()
    assert got.max() == len(rs) - 1 or keys.match_keys(rs, own[-1:])[0] < len(rs) - 1
    for fam in (4, 6):
        assert (got[k["ip_ver"] == fam] >= 0).any() and (got[k["ip_ver"] == fam] == -1).any()
    # IPv4 keys: union bytes 4-15 are not part of the key
    v4 = k["ip_ver"] == 4
    dirty = k[v4].copy()
    dirty["src_ip"][:, 4:] = 0xFF
    dirty["dst_ip"][:, 4:] = 0xFF
    assert np.array_equal(keys.match_keys(rs, dirty), got[v4])


@pytest.mark.parametrize("case", GOLDEN_SMALL)
def test_composition_equals_the_workers_verdicts(case):
    wl, ref = golden_io.load(case)
    k, rc = keys.parse_keys(wl.frames, wl.desc)
    got = keys.match_keys(wl.rules_sorted, k)
    assert (got[rc != 0] == -1).all()
    want = layout.verdict_rule(oracle.run_restated(wl).verdict)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert np.array_equal(got, layout.verdict_rule(ref["verdict"])), "the recorded reference run"
    if oracle.ref_available():
        assert np.array_equal(got, layout.verdict_rule(oracle.run_reference(wl).verdict))
    assert (got >= 0).any() and (case == "config_b_small" or (got == -1).any())


def test_composition_on_control_frames():
    """ARP and consumed NS / NA come out as -1 on both sides."""
    wl, _, sid, _ = gates.control_subset()
    k, rc = keys.parse_keys(wl.frames, wl.desc)
    got = keys.match_keys(wl.rules_sorted, k)
    want = layout.verdict_rule(oracle.run_restated(wl).verdict)
    assert np.array_equal(got, want)
    assert (got[sid >= 0] == -1).all() and (got[sid < 0] >= 0).all()


def test_library_exports_the_key_calls():
    lib = ctypes.CDLL(gpu.LIB_PATH)
    for name in ("upe_gpu_parse_keys", "upe_gpu_match_keys"):
        assert hasattr(lib, name), name
        assert name in gpu.EXPORTED
    assert callable(gpu.GpuWorker.parse_keys) and callable(gpu.GpuWorker.match_keys)
    # argument checks need no GPU: a null context fails with a message, before anything else
    assert gpu.LIB.upe_gpu_parse_keys(None, None, None, 0, None, None, None) == -1
    assert b"null context" in gpu.LIB.upe_gpu_last_error()
    assert gpu.LIB.upe_gpu_match_keys(None, None, None, 0, None, None) == -1
    assert b"null context" in gpu.LIB.upe_gpu_last_error()
