"""CPU: the host side of topk — the oracle helper reproduces the reference chain at k = 4, the k-taking entry points are exported
and refuse bad arguments before the first HIP call (the pointers are dummies that are never dereferenced: every call below is
refused), the parser and the Python entry points validate."""
import ctypes

import pytest
import torch

import topk_oracle as T

NEW = ("knnsvc_concat_reselect_seg_k", "knnsvc_smooth_seg_workspace_bytes_k", "knnsvc_smooth_weights_seg_k")
EINVAL, EWORKSPACE = 1, 2


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


@pytest.fixture(scope="module")
def small():
    """A 300-row pool around six centres, a 23-frame query, f0 with unvoiced frames, 49 harmonics."""
    gen = torch.Generator().manual_seed(3)
    centres = torch.randn(6, 32, generator=gen)
    P = centres[torch.randint(0, 6, (300,), generator=gen)] + 0.3 * torch.randn(300, 32, generator=gen)
    q = P[torch.randint(0, 300, (23,), generator=gen)] + 0.1 * torch.randn(23, 32, generator=gen)
    pool = dict(feats=P, f0=T.f0_track(300, gen, 9), harm=torch.rand(300, 49, generator=gen) * 0.02)
    return dict(feats=q, f0=T.f0_track(23, gen, 5)), pool


@pytest.mark.parametrize("ckpt_type,post_opt", [("mix", "post_opt_0.2"), ("mix", "no_post_opt"), ("wavlm_only", "no_post_opt")])
def test_match_k_at_4_is_the_reference_chain(small, ckpt_type, post_opt):
    from oracle import pipeline_ref
    query, pool = small
    a = pipeline_ref.match(query, pool, ckpt_type, post_opt, return_debug=True)
    b = T.match_k(query, pool, 4, ckpt_type, post_opt)
    for x, y in zip(a[:3], b[:3]):
        assert (x is None and y is None) or torch.equal(x, y)
    assert sorted(a[3]) == sorted(b[3])
    for key in a[3]:
        assert torch.equal(a[3][key], b[3][key]), key
    assert T.match_k(query, pool, 7, ckpt_type, post_opt)[3]["idx_harm"].shape == (23, 7)


def test_walk_margin_replays_the_oracle_and_walk_check_accepts_it():
    from oracle import select_ref
    q, p, idx, sf0, pf0 = T.walk_inputs(12, 200, 64, 3, 5)
    for f0c in ((None, None), (sf0, pf0)):
        ref = select_ref.concat_reselect(idx.clone(), q, p, *f0c, concat_weight=0.2)
        sel, gap, repeated = T.walk_margin(idx.clone(), q, p, *f0c, w=0.2)
        assert torch.equal(sel, ref) and gap > 0 and 0 <= repeated < 12
        assert T.walk_check(idx, ref, q, p, *f0c, w=0.2, tol=0.0) == ([], 0.0)
        wrong = ref.clone()
        wrong[7] = ref[7].flip(0)                                  # descending costs in frame 7 (distinct: gap > 0)
        bad, worst = T.walk_check(idx, wrong, q, p, *f0c, w=0.2, tol=gap / 2)
        assert 7 in bad and worst >= gap


def test_new_symbols_are_exported_and_typed():
    lib = _lib()
    from knn_svc_amd import _lib as L
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert L.ABI_VERSION == lib.knnsvc_abi_version() >= 20          # (20 brought these names; later versions keep them)


def test_workspace_size_by_k():
    lib = _lib()
    lens = [1, 2, 600, 5000]
    tab = _table(lens)
    sizes = [lib.knnsvc_smooth_seg_workspace_bytes_k(tab, len(lens), k) for k in range(0, 10)]
    assert sizes[0] == 0 and sizes[9] == 0
    assert all(a < b for a, b in zip(sizes[1:8], sizes[2:9])) and all(s % 64 == 0 for s in sizes[1:9])
    assert sizes[4] == lib.knnsvc_smooth_seg_workspace_bytes(tab, len(lens))
    # Gram k(2k - 1) + 6k of state + 2k of exchange floats per row, 64 bytes to align the base, rounded up to 64 per segment
    for k in range(1, 9):
        per_row = (k * (2 * k - 1) + 8 * k) * 4
        assert sizes[k] == sum((per_row * n + 64 + 63) // 64 * 64 for n in lens), k
    assert lib.knnsvc_smooth_seg_workspace_bytes_k((ctypes.c_int64 * 3)(0, 3, 3), 2, 5) == 0          # a bad table


def test_k_taking_entry_points_refuse_before_launching():
    lib = _lib()
    d = 256                     # a dummy, 16-byte aligned, never dereferenced
    tab = _table([3, 4])
    walk = lambda k, dim=64, q=d, t=tab, n=2: lib.knnsvc_concat_reselect_seg_k(d, k, q, d, t, n, d, d, 300, dim, d, d, 1, 0.2, d, None)
    smooth = lambda k, ws=1 << 30, t=tab, n=2, out=d: lib.knnsvc_smooth_weights_seg_k(d, k, t, n, d, 300, 64, 64, 0.1, None, 300, out, d, d,
                                                                                       ws, None)
    for call, name in ((walk, b"concat_reselect_seg_k"), (smooth, b"smooth_weights_seg_k")):
        for k in (0, 9, -1):
            assert call(k) == EINVAL
            msg = lib.knnsvc_last_error()
            assert name in msg and f"k = {k}".encode() in msg, msg
    # the LDS bound of the walk, (4k + 2) * dim * 4 <= 150 KB, from both sides at k = 8.  dim 1028 needs 139 808 bytes and passes
    # it (there is no dim <= 1024 limit on this kernel): with a misaligned q the call is refused by the NEXT check, alignment;
    # dim 1132 needs 153 952 bytes and is refused by the bound itself.  Either way nothing is launched.
    assert walk(8, dim=1028, q=d + 4) == EINVAL and b"alignment" in lib.knnsvc_last_error()
    assert walk(8, dim=1132, q=d + 4) == EINVAL and b"LDS" in lib.knnsvc_last_error()
    assert walk(8, dim=1132) == EINVAL and b"LDS" in lib.knnsvc_last_error()
    assert walk(1, dim=7680) == EINVAL and b"LDS" in lib.knnsvc_last_error()            # 6 * 7680 * 4 = 180 KB
    assert walk(3, dim=62) == EINVAL                                                    # dim % 4
    assert walk(3, q=d + 4) == EINVAL and b"alignment" in lib.knnsvc_last_error()
    # a short workspace
    for k in (1, 5, 8):
        need = lib.knnsvc_smooth_seg_workspace_bytes_k(tab, 2, k)
        assert need > 0 and smooth(k, ws=need - 1) == EWORKSPACE
        msg = lib.knnsvc_last_error()
        assert b"smooth_weights_seg_k" in msg and b"workspace" in msg, msg
    assert smooth(5, out=d + 2) == EINVAL and b"aligned" in lib.knnsvc_last_error()
    # a bad table
    for bad, n in (((ctypes.c_int64 * 3)(0, 3, 3), 2), ((ctypes.c_int64 * 2)(1, 3), 1), (tab, 0), (_table([1] * 65), 65)):
        assert walk(5, t=bad, n=n) == EINVAL and b"concat_reselect_seg_k" in lib.knnsvc_last_error()
        assert smooth(5, t=bad, n=n) == EINVAL and b"smooth_weights_seg_k" in lib.knnsvc_last_error()
    # uniform gather: any k is taken now, a mode other than 0 / 1 is not (refused before the launch)
    assert lib.knnsvc_weighted_gather(d, None, 5, 3, d, 64, 64, 2, d, None) == EINVAL and b"mean_mode" in lib.knnsvc_last_error()


def test_parser_and_python_side_validation():
    from knn_svc_amd import matching as M
    from knn_svc_amd.inference import build_parser
    a = build_parser().parse_args(["s", "t", "--use_topk", "true", "--topk", "6"])
    assert a.use_topk is True and a.topk == 6
    assert build_parser().parse_args(["s", "t"]).use_topk is False
    assert "(extension)" in [x for x in build_parser()._actions if x.dest == "use_topk"][0].help
    q, f0 = torch.zeros(5, 8), torch.zeros(5)
    for bad in (9, 0, -1, 2.5, True):
        with pytest.raises(ValueError):
            M.match_features_many([q], [f0], torch.zeros(40, 8), torch.zeros(40), torch.zeros(40, 49), "mix", "no_post_opt", topk=bad)
        with pytest.raises(ValueError):
            M.match_features(q, f0, torch.zeros(40, 8), torch.zeros(40), torch.zeros(40, 49), "mix", "no_post_opt", topk=bad)
    assert M.resolve_topk(None) == 4 and M.resolve_topk(8) == 8 and M.resolve_topk(1) == 1
    from knn_svc_amd import serving
    with pytest.raises(ValueError):
        serving.BatchConverter(None, None, topk=9)
    # the reference-named entry point: refused before any file is read, and only when the caller opted in
    with pytest.raises(ValueError):
        M.match_at_inference_time("/nonexistent/a.wav", "/nonexistent/b.wav", None, topk=9, prioritize_f0=True, use_topk=True)


def test_ops_refuse_k_outside_1_to_8():
    from knn_svc_amd import ops
    from knn_svc_amd._lib import KnnSvcError
    z = torch.zeros(3, 9, dtype=torch.int64)
    with pytest.raises(KnnSvcError):
        ops.concat_reselect(z, None, None, None, None)
