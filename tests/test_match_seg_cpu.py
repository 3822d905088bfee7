"""CPU: the host side of the segmented match-stage entry points (knnsvc_*_seg).  The segment table is validated before the first
HIP call, so a bad table, a bad segment count or a short workspace is refused on a machine without a GPU; the pointers are
dummies that are never dereferenced."""
import ctypes

import pytest

LENS = [1, 2, 600, 1100, 1600, 5000]


def _lib():
    import __graft_entry__ as g
    g.build()
    from knn_svc_amd import _lib
    return _lib.load()


def _table(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return (ctypes.c_int64 * len(off))(*off)


def _raw(vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def test_seg_workspace_bytes():
    lib = _lib()
    got = lib.knnsvc_smooth_seg_workspace_bytes(_table(LENS), len(LENS))
    assert got >= sum(lib.knnsvc_smooth_workspace_bytes(n) for n in LENS)
    assert got % 64 == 0
    for perm in ([5000, 1, 1600, 2, 1100, 600], LENS[::-1]):
        assert lib.knnsvc_smooth_seg_workspace_bytes(_table(perm), len(perm)) == got
    assert lib.knnsvc_smooth_seg_workspace_bytes(_table([7]), 1) >= lib.knnsvc_smooth_workspace_bytes(7)
    for bad, n in ((_raw([0, 3, 3]), 2), (_raw([1, 3]), 1), (_raw([0, 5, 2]), 2), (_table([1]), 0), (_table([1] * 65), 65)):
        assert lib.knnsvc_smooth_seg_workspace_bytes(bad, n) == 0


BAD_TABLES = {
    "n_seg = 0": (_table([3, 4]), 0),
    "n_seg = 65": (_table([2] * 65), 65),
    "host_seg[0] = 1": (_raw([1, 4, 9]), 2),
    "empty segment": (_raw([0, 4, 4, 9]), 3),
    "descending": (_raw([0, 9, 4]), 2),
}


def _calls(lib, tab, n, ws_bytes=1 << 30):
    d = 256                 # a dummy, 16-byte aligned, never dereferenced: every check below fails (or would launch) before a read
    return {
        "log_f0_median_seg": lambda: lib.knnsvc_log_f0_median_seg(d, tab, n, d, d, None),
        "shift_f0_seg": lambda: lib.knnsvc_shift_f0_seg(d, tab, n, d, d, d, None),
        "concat_reselect_seg": lambda: lib.knnsvc_concat_reselect_seg(d, d, d, tab, n, d, d, 300, 64, d, d, 1, 0.2, d, None),
        "smooth_weights_seg": lambda: lib.knnsvc_smooth_weights_seg(d, tab, n, d, 300, 64, 64, 0.1, None, 300, d, d, d, ws_bytes, None),
    }


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_seg_entry_points_refuse_a_bad_table_before_launching(case):
    lib = _lib()
    tab, n = BAD_TABLES[case]
    for name, call in _calls(lib, tab, n).items():
        rc = call()
        msg = lib.knnsvc_last_error()
        assert rc != 0 and name.encode() in msg, (case, name, rc, msg)


def test_smooth_weights_seg_refuses_a_short_workspace():
    lib = _lib()
    tab = _table(LENS)
    need = lib.knnsvc_smooth_seg_workspace_bytes(tab, len(LENS))
    rc = _calls(lib, tab, len(LENS), ws_bytes=need - 1)["smooth_weights_seg"]()
    msg = lib.knnsvc_last_error()
    assert rc == 2 and b"workspace" in msg, (rc, msg)          # KNNSVC_EWORKSPACE


def test_seg_entry_points_refuse_bad_sizes_and_null_pointers():
    lib = _lib()
    tab = _table([3, 4])
    d = 256
    assert lib.knnsvc_concat_reselect_seg(d, d, d, tab, 2, d, d, 300, 62, d, d, 0, 0.2, d, None) != 0          # dim % 4
    assert lib.knnsvc_concat_reselect_seg(d, d + 4, d, tab, 2, d, d, 300, 64, d, d, 0, 0.2, d, None) != 0      # alignment
    assert b"alignment" in lib.knnsvc_last_error()
    assert lib.knnsvc_concat_reselect_seg(d, d, d, tab, 2, d, d, 300, 64, None, None, 1, 0.2, d, None) != 0    # f0 variant without f0
    assert lib.knnsvc_log_f0_median_seg(None, tab, 2, d, d, None) != 0
    assert lib.knnsvc_log_f0_median_seg(d, None, 2, d, d, None) != 0
    assert lib.knnsvc_shift_f0_seg(d, tab, 2, None, d, d, None) != 0
    assert lib.knnsvc_smooth_weights_seg(d, tab, 2, d, 300, 64, 32, 0.1, None, 300, d, d, d, 1 << 20, None) != 0   # ld < dim
    assert lib.knnsvc_smooth_weights_seg(d, tab, 2, d, 300, 64, 64, 0.1, None, 300, d + 4, d, d, 1 << 20, None) != 0
    assert b"aligned" in lib.knnsvc_last_error()


def test_single_entry_points_answer_under_their_own_names():
    """The single-sequence entry points are the one-segment case of the segmented ones, but speak as themselves: their own
    name in the message, their own workspace size.  Per row the workspace is the Gram matrix's 28 off-diagonal entries + 6 float4
    of optimiser state + 2 float4 of exchange buffer = 60 floats (smooth.hip, ws_floats), then 64 bytes to align the base: 240 n +
    64 — the value the function returned before the single call became a one-segment call (the 68 floats / 272 bytes per row some
    notes quote are the 36-entry Gram layout of an older version)."""
    lib = _lib()
    d = 256
    calls = {
        "log_f0_median": lambda: lib.knnsvc_log_f0_median(d, 0, d, d, None),
        "shift_f0": lambda: lib.knnsvc_shift_f0(d, 0, d, d, d, None),
        "concat_reselect": lambda: lib.knnsvc_concat_reselect(d, d, d, 0, d, d, 300, 64, d, d, 1, 0.2, d, None),
        "smooth_weights": lambda: lib.knnsvc_smooth_weights(d, 0, d, 300, 64, 64, 0.1, None, 300, d, d, d, 1 << 30, None),
    }
    for name, call in calls.items():
        rc = call()
        msg = lib.knnsvc_last_error()
        assert rc != 0 and name.encode() in msg and b"_seg" not in msg, (name, rc, msg)
    for n in (1, 7, 600, 5000):
        need = lib.knnsvc_smooth_workspace_bytes(n)
        assert need == (28 + 6 * 4 + 2 * 4) * 4 * n + 64 == 240 * n + 64, (n, need)
        rc = lib.knnsvc_smooth_weights(d, n, d, 300, 64, 64, 0.1, None, 300, d, d, d, need - 1, None)
        msg = lib.knnsvc_last_error()
        assert rc == 2 and b"smooth_weights:" in msg and b"workspace" in msg, (n, rc, msg)          # KNNSVC_EWORKSPACE
    assert lib.knnsvc_smooth_workspace_bytes(0) == 0


def test_segment_chunks_of_the_wrapper():
    """ops._seg_chunks: a table of more than 64 segments becomes consecutive calls with tables that start at 0."""
    from knn_svc_amd import ops
    seg = [0]
    for i in range(70):
        seg.append(seg[-1] + 1 + i % 3)
    chunks = ops._seg_chunks(seg)
    assert [(a, r0, len(t) - 1) for a, r0, t in chunks] == [(0, 0, 64), (64, seg[64], 6)]
    assert list(chunks[1][2]) == [v - seg[64] for v in seg[64:]]
    assert list(chunks[0][2]) == seg[:65]


def test_match_route_switch_defaults_and_environment(monkeypatch):
    """The default route stays "lanes"; KNNSVC_MATCH / KNNSVC_MATCH_BATCH set the defaults, an argument wins, junk is refused."""
    from knn_svc_amd import matching as M
    monkeypatch.delenv("KNNSVC_MATCH", raising=False); monkeypatch.delenv("KNNSVC_MATCH_BATCH", raising=False)
    assert M.match_mode() == "lanes" and M.match_batch_size() == M.MATCH_BATCH_DEFAULT
    monkeypatch.setenv("KNNSVC_MATCH", "segmented"); monkeypatch.setenv("KNNSVC_MATCH_BATCH", "8")
    assert M.match_mode() == "segmented" and M.match_batch_size() == 8
    assert M.match_mode("lanes") == "lanes" and M.match_batch_size(4) == 4
    with pytest.raises(ValueError):
        M.match_mode("streams")
    with pytest.raises(ValueError):
        M.match_batch_size(0)
