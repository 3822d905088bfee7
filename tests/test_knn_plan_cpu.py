"""The f16x2 search's host plan (knn_svc_amd/ops.py: knn_plan): pool chunks, routes, query blocks, epochs, the one fill — no GPU.
The expected numbers are literals: the previous host path's expressions (knn_pool_chunks, the loops of _knn_topk_gemm and
_knn_fused_chunk) evaluated once by hand, never knn_plan's own output."""
import random

import pytest

from knn_svc_amd import ops


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    monkeypatch.delenv("KNNSVC_KNN_FUSED", raising=False)


def _shape(plan):
    """[((p0, p1), route, [(q0, m), ...]), ...]"""
    return [((c.p0, c.p1), "fused" if c.fused else "dot", [(b.q0, b.m) for b in c.blocks]) for c in plan.chunks]


def _epochs(plan):
    return [[list(b.epochs) for b in c.blocks] for c in plan.chunks]


def test_north_star_point_is_one_fused_block_whose_workspace_rides_in_the_fill():
    plan = ops.knn_plan(1500, 30000, 1024, 32)
    assert _shape(plan) == [((0, 30000), "fused", [(0, 1500)])]
    assert _epochs(plan) == [[[(0, 42), (42, 118)]]]
    assert plan.fill_words == 129192 and plan.chunks[0].blocks[0].fill == 129192
    assert ops.knn_search_fill(1500, 30000, 1024) == 129192


@pytest.mark.parametrize("nq,npool,route,fill", [(255, 30000, "dot", 0), (256, 8191, "dot", 0), (256, 8192, "fused", 16928)])
def test_route_thresholds(nq, npool, route, fill):
    plan = ops.knn_plan(nq, npool, 1024, 32)
    assert _shape(plan) == [((0, npool), route, [(0, nq)])]
    assert plan.fill_words == fill
    if route == "dot":
        assert plan.chunks[0].blocks[0].epochs == () and plan.chunks[0].npad == -(-npool // 4) * 4


def test_a_second_pool_chunk_ends_the_shared_fill():
    one, two = ops.knn_plan(300, 262016, 1024, 32), ops.knn_plan(300, 262017, 1024, 32)
    assert _shape(one) == [((0, 262016), "fused", [(0, 300)])] and one.fill_words == 27064
    assert _epochs(one) == [[[(0, 44), (44, 176), (176, 704), (704, 1024)]]]
    assert _shape(two) == [((0, 131009), "fused", [(0, 300)]), ((131009, 262017), "fused", [(0, 300)])]
    assert _epochs(two) == [[[(0, 44), (44, 176), (176, 512)]]] * 2
    assert two.fill_words == 0 and [c.blocks[0].fill for c in two.chunks] == [27064, 27064]


def test_a_second_query_block_ends_the_shared_fill():
    one, two = ops.knn_plan(32768, 30000, 1024, 32), ops.knn_plan(32769, 30000, 1024, 32)
    assert _shape(one) == [((0, 30000), "fused", [(0, 32768)])] and one.fill_words == 331776
    assert _shape(two) == [((0, 30000), "fused", [(0, 32768), (32768, 1)])] and two.fill_words == 0
    assert _epochs(two) == [[[(0, 4), (4, 16), (16, 64), (64, 118)], [(0, 44), (44, 118)]]]
    assert [b.fill for b in two.chunks[0].blocks] == [331776, 122]


def test_dot_route_blocks_keep_the_dot_matrix_within_the_bound():
    plan = ops.knn_plan(24000, 180000, 1024, 32, allow_fused=False)
    (bounds, route, blocks), = _shape(plan)
    assert bounds == (0, 180000) and route == "dot" and plan.fill_words == 0
    assert blocks == [(q0, min(1408, 24000 - q0)) for q0 in range(0, 24000, 1408)] and len(blocks) == 18 and blocks[-1] == (23936, 64)


@pytest.mark.parametrize("max_blocks,epochs,fill", [(0, [(0, 21), (21, 84), (84, 118)], 132384), (192, [(0, 16), (16, 64), (64, 118)], 102384)])
def test_the_grid_cap_moves_the_first_epoch_and_with_it_the_fill(max_blocks, epochs, fill):
    plan = ops.knn_plan(3000, 30000, 1024, 32, max_blocks=max_blocks)
    assert _shape(plan) == [((0, 30000), "fused", [(0, 3000)])] and _epochs(plan) == [[epochs]]
    assert plan.fill_words == fill == ops.knn_search_fill(3000, 30000, 1024, max_blocks)


def test_at_dim_8192_the_split_image_cuts_the_queries_and_nothing_is_folded():
    """The previous knn_search_fill returned a size here (32600 * 8192 < 2^28) that the executor then did not use."""
    plan = ops.knn_plan(32600, 30000, 8192, 32)
    assert _shape(plan) == [((0, 30000), "fused", [(0, 32512), (32512, 88)])]
    assert _epochs(plan) == [[[(0, 4), (4, 16), (16, 64), (64, 118)], [(0, 44), (44, 118)]]]
    assert [b.fill for b in plan.chunks[0].blocks] == [329184, 7952]
    assert plan.fill_words == 0 and ops.knn_search_fill(32600, 30000, 8192) == 0


def test_every_cap_follows_the_one_bound(monkeypatch):
    monkeypatch.setattr(ops, "KNN_RSRC_BYTES", 1 << 24)
    assert ops.knn_pool_chunks(20000, 256) == [(0, 10000), (10000, 20000)]
    plan = ops.knn_plan(768, 20000, 256, 32, max_blocks=16)
    assert _shape(plan) == [((0, 10000), "fused", [(0, 512), (512, 256)]), ((10000, 20000), "fused", [(0, 512), (512, 256)])]
    assert _epochs(plan) == [[[(0, 8), (8, 40)], [(0, 16), (16, 40)]]] * 2
    assert [b.fill for b in plan.chunks[0].blocks] == [9280, 8736] and plan.fill_words == 0
    dot = ops.knn_plan(768, 20000, 256, 32, allow_fused=False)
    assert _shape(dot) == [((0, 10000), "dot", [(0, 384), (384, 384)]), ((10000, 20000), "dot", [(0, 384), (384, 384)])]
    assert [c.npad for c in dot.chunks] == [10000, 10000]


def test_both_fused_switches_send_every_chunk_to_the_dot_matrix(monkeypatch):
    with ops.fused_off():
        assert _shape(ops.knn_plan(768, 20000, 256, 32)) == [((0, 20000), "dot", [(0, 768)])]
        assert ops.knn_search_fill(768, 20000, 256) == 0
    assert ops.knn_plan(768, 20000, 256, 32).chunks[0].fused
    monkeypatch.setenv("KNNSVC_KNN_FUSED", "0")
    plan = ops.knn_plan(1500, 30000, 1024, 32)
    assert _shape(plan) == [((0, 30000), "dot", [(0, 1500)])] and plan.fill_words == 0
    assert ops.knn_search_fill(1500, 30000, 1024) == 0


def test_a_prepared_pools_bounds_are_the_plans_bounds():
    bounds = [(0, 9000), (9000, 20000)]
    plan = ops.knn_plan(300, 20000, 256, 32, chunk_bounds=bounds)
    assert [(c.p0, c.p1) for c in plan.chunks] == bounds and [c.fused for c in plan.chunks] == [True, True]
    assert plan.fill_words == 0
    with pytest.raises(ops.KnnSvcError):
        ops.knn_plan(300, 20000, 256, 32, chunk_bounds=[(0, 19990), (19990, 20000)])


@pytest.mark.parametrize("dim", [256, 768, 1024])
def test_every_buffer_a_plan_implies_is_within_the_bound(dim):
    """What the numbers exist for.  (Not below dim 128: the dot route's floor of 128 query rows knowingly exceeds the bound there.)"""
    rng = random.Random(dim)
    R, k = ops.KNN_RSRC_BYTES, 32
    points = [(100000, 3000000), (1, 32), (256, 8192), (32768, 30000), (32769, 3000000)]
    points += [(rng.randint(1, 100000), rng.randint(k, 3000000)) for _ in range(300)]
    points += [(rng.randint(1, 2000), rng.randint(k, 20000)) for _ in range(100)]
    for nq, npool in points:
        for allow_fused in (True, False):
            plan = ops.knn_plan(nq, npool, dim, k, allow_fused=allow_fused, max_blocks=rng.choice((0, 16, 192)))
            at = (nq, npool, dim, allow_fused)
            assert plan.chunks[0].p0 == 0 and plan.chunks[-1].p1 == npool, at
            assert all(a.p1 == b.p0 for a, b in zip(plan.chunks, plan.chunks[1:])), at
            for c in plan.chunks:
                rows = c.p1 - c.p0
                assert rows >= k and rows * dim * 4 < R and c.npad == -(-rows // 4) * 4, at
                assert c.fused == (allow_fused and nq >= ops.KNN_FUSED_MIN_Q and rows >= ops.KNN_FUSED_MIN_P), at
                assert c.blocks[0].q0 == 0 and c.blocks[-1].q0 + c.blocks[-1].m == nq, at
                assert all(a.q0 + a.m == b.q0 for a, b in zip(c.blocks, c.blocks[1:])), at
                for b in c.blocks:
                    assert b.m > 0 and b.m * dim * 4 < R, at
                    if c.fused:
                        assert b.m * ops.KNN_FUSED_CAP * 8 <= R, at
                        assert b.epochs[0][0] == 0 and b.epochs[-1][1] == -(-rows // 256), at
                        assert b.fill == b.m * (2 + 2 * b.epochs[0][1]) + 32 * -(-b.m // 256), at
                    else:
                        assert b.m * c.npad * 4 <= R and b.epochs == () and b.fill == 0, at
            one = len(plan.chunks) == 1 and plan.chunks[0].fused and len(plan.chunks[0].blocks) == 1
            assert (plan.fill_words > 0) == one, at
            if one:
                assert plan.fill_words == plan.chunks[0].blocks[0].fill, at
