"""Host logic of the fused kNN route's epoch plan (knn_svc_amd/ops.py: knn_epochs) — no GPU."""
import pytest

from knn_svc_amd import ops


@pytest.mark.parametrize("nq,npc,blocks", [(1500, 30000, 256), (300, 30000, 256), (3000, 30000, 192), (24000, 180000, 256),
                                           (257, 8197, 256), (32768, 262143, 256), (1, 300, 8)])
def test_epochs_cover_every_column_tile_once_in_growing_steps(nq, npc, blocks):
    ep = ops.knn_epochs(nq, npc, blocks)
    gy = -(-npc // 256)
    assert ep[0][0] == 0 and ep[-1][1] == gy
    for (a0, a1), (b0, b1) in zip(ep, ep[1:]):
        assert a1 == b0 and a0 < a1 and b0 < b1
    e0 = ep[0][1]
    assert e0 == gy or 4 <= e0 <= ops.KNN_COLD_TILES_MAX
    assert e0 * 48 <= ops.KNN_FUSED_CAP                       # ~45 survivors per (row, cold tile) fit the candidate buffer
    for (a0, a1) in ep[1:]:
        assert a1 <= a0 * ops.KNN_EPOCH_GROWTH or a1 == gy     # thresholds are never staler than one growth step


def test_north_star_point_is_one_cold_round_and_one_warm_epoch():
    assert ops.knn_epochs(1500, 30000, 256) == [(0, 42), (42, 118)]       # 6 x 42 = 252 workgroups, then 6 x 76 = 456


def _window_points(dim):
    R = ops.KNN_RSRC_BYTES
    p_cap = (R - 1) // (dim * 4) // 128 * 128
    top = (R - 1) // (dim * 4)                                  # the largest pool whose fp32 rows stay below the bound (1 GiB)
    return p_cap, top, [p_cap - 1, p_cap, p_cap + 1, top, R // (4 * dim)]


@pytest.mark.parametrize("dim", [256, 512, 768, 1024, 2048])
def test_pool_chunk_plan_and_the_one_fill_agree_at_the_chunk_boundary(dim, monkeypatch):
    """the search's one pre-zeroed first-epoch workspace may only go to a search of ONE pool chunk (ops.knn_search_fill);
    between p_cap (prepare_knn_pool's chunk size) and KNN_RSRC_BYTES / (4 dim) the pool splits into two chunks, which must each get
    their own.  The plan: balanced chunks of at least k rows that cover [0, npool) once."""
    monkeypatch.delenv("KNNSVC_KNN_FUSED", raising=False)
    p_cap, top, points = _window_points(dim)
    assert p_cap < top
    for npool in points:
        chunks = ops.knn_pool_chunks(npool, dim)
        assert chunks[0][0] == 0 and chunks[-1][1] == npool
        assert all(a1 == b0 for (_, a1), (b0, _) in zip(chunks, chunks[1:]))
        sizes = [b - a for a, b in chunks]
        assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 32 and max(sizes) <= p_cap
        assert len(chunks) == (1 if npool <= p_cap else 2), (npool, chunks)
        nq = 300
        assert nq >= ops.KNN_FUSED_MIN_Q and npool >= ops.KNN_FUSED_MIN_P
        fill = ops.knn_search_fill(nq, npool, dim)
        assert (fill > 0) == (len(chunks) == 1), (dim, npool, fill, chunks)
