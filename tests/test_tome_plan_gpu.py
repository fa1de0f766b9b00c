"""GPU tests of tome_plan_kernel: the plan of the kernel route must EQUAL the
torch route's (ops.tome_plan(..., native=False)) on CPU copies of the same
inputs, table by table. Integer output, an exact oracle: no tolerance.
"""
import pytest
import torch

from sdwd_amd import ops

pytestmark = pytest.mark.gpu

# less than one wave; odd edges; several waves with partial last waves; the
# largest square row; the largest src count the token bound admits (h = 3)
GRIDS = [(2, 2), (9, 11), (18, 14), (24, 24), (128, 128), (3, 5461)]
FAMILIES = ["random", "equal", "four", "one_dst", "special", "clamp"]
NAMES = ("slot", "unm_tok", "seg_start", "members")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def _inputs(family, bsz, h, w, seed=0):
    """CPU (node_max fp32, node_idx int32) [bsz, Ns]; rows differ."""
    src, dst = ops.tome_partition(h, w)
    ns, nd = src.numel(), dst.numel()
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    nm = torch.rand(bsz, ns, generator=g) * 2 - 1
    ni = torch.randint(0, nd, (bsz, ns), generator=g, dtype=torch.int32)
    if family == "equal":  # pure tie-breaking by position
        nm = torch.full((bsz, ns), 0.25)
    elif family == "four":  # ties straddle the threshold for most r
        pick = torch.randint(0, 4, (bsz, ns), generator=g)
        nm = torch.tensor([-0.5, 0.0, 0.5, 0.75])[pick]
    elif family == "one_dst":  # one segment of length r
        ni = torch.full((bsz, ns), nd // 2, dtype=torch.int32)
    elif family == "special":
        vals = torch.tensor([float("nan"), float("inf"), float("-inf"),
                             0.0, -0.0]).repeat(3)
        for b in range(bsz):
            at = torch.randint(0, ns, (vals.numel(),), generator=g)
            nm[b, at] = vals
    elif family == "clamp":
        ni[:, ::3] = -1
        ni[:, 1::3] = nd + 5
    return nm, ni


def _assert_equal(got, want, tag):
    for name, a, b in zip(NAMES, got.tensors(), want.tensors()):
        assert a.dtype == torch.int32 and a.shape == b.shape, (tag, name)
        assert torch.equal(a.cpu(), b), (tag, name)


@pytest.mark.parametrize("bsz", [1, 3])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("hw", GRIDS)
def test_equals_torch_route(dev, hw, family, bsz):
    h, w = hw
    n = h * w
    nm, ni = _inputs(family, bsz, h, w)
    nmg, nig = nm.to(dev), ni.to(dev)
    assert ops.tome_plan_supported(nmg, nig, h, w)
    for r in (0, 1, n // 4, n // 2, nm.shape[1]):
        want = ops.tome_plan(nm, ni, h, w, r, native=False)
        got = ops.tome_plan(nmg, nig, h, w, r)
        assert got.slot.is_cuda and got.dst_tok.is_cuda
        _assert_equal(got, want, f"{hw} {family} B={bsz} r={r}")


def test_graph_replay_equals_eager(dev):
    h, w, bsz = 24, 24, 2
    r = h * w // 2
    nm, ni = _inputs("four", bsz, h, w)
    nmg, nig = nm.to(dev), ni.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.tome_plan(nmg, nig, h, w, r)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan = ops.tome_plan(nmg, nig, h, w, r)
    for seed, family in ((1, "random"), (2, "special"), (3, "one_dst")):
        nm, ni = _inputs(family, bsz, h, w, seed)
        nmg.copy_(nm)
        nig.copy_(ni)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.tome_plan(nmg, nig, h, w, r)
        for name, a, b in zip(NAMES, plan.tensors(), eager.tensors()):
            assert torch.equal(a, b), (family, name)
        _assert_equal(plan, ops.tome_plan(nm, ni, h, w, r, native=False),
                      f"replay {family}")


def test_support_boundary(dev):
    nm, ni = _inputs("random", 1, 18, 14)
    assert not ops.tome_plan_supported(nm, ni, 18, 14)  # CPU tensors
    h, w = 130, 128  # above the kernel's 16384 tokens: the torch route
    nm, ni = _inputs("four", 2, h, w)
    nmg, nig = nm.to(dev), ni.to(dev)
    assert not ops.tome_plan_supported(nmg, nig, h, w)
    r = h * w // 2
    _assert_equal(ops.tome_plan(nmg, nig, h, w, r),
                  ops.tome_plan(nm, ni, h, w, r, native=False), "130x128")
