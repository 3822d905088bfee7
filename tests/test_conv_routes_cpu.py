"""CPU: the route table of tests/conv_routes_common.py against the dispatcher itself, asked through its host-only route entry
(ops.conv_route / ops.conv_tags: nothing is launched).  A kernel tag the dispatcher can report without a row — a new route
nobody compares with fp64 — fails here, before any GPU run; so does a row the dispatcher sends elsewhere than it says, or whose
shape does not have the properties the row is about."""
import pytest
import torch

from knn_svc_amd import ops
from tests import conv_routes_common as R


def test_every_tag_the_dispatcher_can_report_has_a_row():
    tags = ops.conv_tags()
    assert len(tags) >= 30, sorted(tags)            # every family is there
    table = {c.tag for c in R.CASES}
    assert table == tags, f"without a row: {sorted(tags - table)}; rows for no kernel: {sorted(table - tags)}"


def test_bucketed_rows_name_kernels_of_the_table():
    assert {c.tag for c, *_ in R.DYN_CASES} <= {c.tag for c in R.CASES}
    for c, per, count, bucket in R.DYN_CASES:
        assert c.batches == 1 and 0 < count < bucket and c.m // bucket == per
        assert R.route(R.dyn_exact(c, per, count, bucket))[0] == c.tag          # the exact-length launch takes the same kernel


@pytest.mark.parametrize("case", R.CASES + [c for c, *_ in R.DYN_CASES], ids=lambda c: c.id)
def test_row_reaches_its_route_by_the_dispatch_rules(case):
    """The dispatcher sends the row's descriptors where the row says, and the row's shape has the properties it relies on."""
    tag, epi = R.route(case)
    assert tag == case.tag
    if case.branches:
        assert case.epi is None and 2 <= len(case.branches) <= 4
        assert len({k for k, _ in case.branches}) == len(case.branches)     # different taps per descriptor
        assert epi in ("patch", "lane")                                     # the windowed kernels' epilogues
    else:
        assert case.epi == epi
    for c in case.descs():
        assert c.t_in_ > 0 and c.rows > 0
        if c.family != "fp32" or c.tag.endswith("v8"):
            assert c.cin % 32 == 0                              # the buffer-load fast path
        if c.tag.endswith("v4"):
            assert c.cin % 4 == 0 and c.cin % 32 != 0
        if c.tag.endswith("v1"):
            assert c.cin % 4 != 0
        if c.split:
            assert (c.cin * c.k) % 32 == 0                      # attach_split takes the weights
        if c.epi == "patch":
            assert c.n % 4 == 0 and c.ldo % 4 == 0 and c.act == R.ACT_NONE and not c.accumulate and c.div == 1.0
        if c.x_split:
            assert c.a_slope == 1.0 and c.split == "f16x2"
        if c.convt:
            assert c.n == c.convt[0] * c.convt[1] and c.dil == -1 and c.stride == 1
        assert c.ldo > c.width and (not c.resid or c.ldr != c.ldo)      # a wider buffer, and a residual of another pitch
    # ragged on purpose (rows below one tile are ragged by themselves)
    tile_n = 256 if case.tag.startswith("Q") else 128 if "128" in case.tag or "160" in case.tag else 64 if "64" in case.tag else 32
    assert case.n % tile_n != 0 or case.convt or case.branches or case.tag == "W64P", (case.n, tile_n)
    assert case.m % 32 != 0 or case.id.endswith("-dyn")


def test_knobs_are_used_only_where_the_route_needs_one():
    with_knob = {c.id for c in R.CASES if c.env}
    assert with_knob == {"W128D-generic-epilogue", "F64-win-off"}


def test_reference_matches_a_direct_sum():
    """The fp64 reference against the header's formula written out (out[m, n] = sum_{tap, c} A(m, tap, c) W[n][tap * cin + c]) on
    a small dilated row and a small transposed one, and e32 in the range the tolerance is built on."""
    c = R.replace(R.BY_ID["W64-shorter-than-halo"], m=9, a_slope=0.1, act=R.ACT_TANH, resid=True, accumulate=True, div=3.0)
    inp = R.make_inputs(c)
    ref = R.reference(c, inp, torch.float64)
    x = torch.nn.functional.leaky_relu(inp["x"].double()[0], 0.1)
    w = inp["w"].double()
    out = torch.zeros(c.m, c.n, dtype=torch.float64)
    for m in range(c.m):
        for tap in range(c.k):
            t = m * c.stride + tap * c.dil - c.pad_
            if 0 <= t < c.t_in_:
                out[m] += w[:, :, tap] @ x[t]
    out = ((torch.tanh(out + inp["bias"].double()) + inp["resid"].double()[0]) + inp["prev"].double()[0]) / 3.0
    assert float((out - ref[0]).abs().max()) < 1e-12

    c = R.replace(R.BY_ID["F32-convt"], m=12)
    inp = R.make_inputs(c)
    ref = R.reference(c, inp, torch.float64)
    u, cout = c.convt
    x = torch.nn.functional.leaky_relu(inp["x"].double()[0], 0.1)
    w = inp["w"].double()                                       # [cin, cout, k * u]
    out = torch.zeros(c.rows, cout, dtype=torch.float64)
    for q in range(c.m):                                        # GEMM row q, phase p -> output row q * u + p - pad
        for p in range(u):
            o = q * u + p - (c.k * u - u) // 2
            if not 0 <= o < c.rows:
                continue
            for r in range(c.k):
                if 0 <= q - r < c.t_in_:
                    out[o] += x[q - r] @ w[:, :, p + r * u]
    out = out + inp["bias"].double()
    assert float((out - ref[0]).abs().max()) < 1e-12

    _, ref64, e32, scale = R.prepared(R.BY_ID["W64"])
    assert 2e-7 < e32 < 5e-6 and 1.0 < scale < 20.0
