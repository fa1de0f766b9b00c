"""fp64 reference of token merging (steps 1-4 of docs/kernels.md, "tome.hip")
from the bf16 inputs, written with plain loops and numpy so that it shares
no code with sdwd_amd.ops, and the error bound of the match.

Bound. A score is <a, b> / (|a| |b|) over C exact bf16 products (a bf16
product is exact in fp32) accumulated in fp32. Under any rounding mode and
any summation order the accumulated sum is within C * 2^-23 * sum|a_d b_d|
of the exact one to first order, and sum|a_d b_d| <= |a||b| (Cauchy-Schwarz),
so the dot product contributes C * 2^-23 to the score. The two norms (fp32
sums of squares of the same length, whose relative error the square root
halves), the rsqrt and the two scaling multiplies are covered by the extra
16 units:

    E0(C) = (C + 16) * 2^-23.

Two candidates closer than 2 * E0 cannot be told apart by a conforming
implementation; everything else is exact.
"""
import numpy as np
import torch

NORM_FLOOR = 2.0 ** -80

# (h, w) -> what it exercises (tile = 64 dst rows, block = 128 src rows)
SHAPES = {
    (16, 16): "exactly one dst tile; a ragged second src block",
    (18, 14): "ragged dst tile",
    (24, 24): "three dst tiles, the last with 16 rows",
    (9, 11): "odd tail row and column are src",
}
BATCH = 2
WIDTH = 320


def e0(c: int) -> float:
    return (c + 16) * 2.0 ** -23


def partition(h: int, w: int):
    """(src_tok, dst_tok) as ascending int64 numpy arrays."""
    src, dst = [], []
    for y in range(h):
        for x in range(w):
            is_dst = (y % 2 == 0 and x % 2 == 0
                      and y < 2 * (h // 2) and x < 2 * (w // 2))
            (dst if is_dst else src).append(y * w + x)
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)


def merge_count(h: int, w: int, ratio: float) -> int:
    src, _ = partition(h, w)
    return min(len(src), int(h * w * ratio))


def scores(x: torch.Tensor, h: int, w: int) -> np.ndarray:
    """fp64 cosine scores [B, Ns, Nd] of x [B, h*w, C] (any float dtype)."""
    src, dst = partition(h, w)
    xd = x.detach().cpu().double().numpy()
    a, b = xd[:, src], xd[:, dst]
    ra = 1.0 / np.sqrt(np.maximum((a * a).sum(-1), NORM_FLOOR))
    rb = 1.0 / np.sqrt(np.maximum((b * b).sum(-1), NORM_FLOOR))
    return np.einsum("bic,bjc->bij", a, b) * ra[:, :, None] * rb[:, None, :]


def match(s: np.ndarray):
    """(node_max [B,Ns], node_idx [B,Ns]) of fp64 scores; np.argmax returns
    the first (lowest) maximiser."""
    return s.max(-1), s.argmax(-1)


def top_two_gap(s: np.ndarray) -> np.ndarray:
    """[B, Ns]: best score minus the best score at any OTHER dst index."""
    part = np.sort(s, axis=-1)
    return part[..., -1] - part[..., -2]


def plan(node_max, node_idx, h: int, w: int, r: int):
    """Steps 3 and 4 for arrays [B, Ns]: dict of int64 numpy arrays slot
    [B,N], unm_tok [B,Ns-r], seg_start [B,Nd+1], members [B,r]."""
    src, dst = partition(h, w)
    ns, nd, n = len(src), len(dst), h * w
    node_max = np.asarray(node_max)
    node_idx = np.asarray(node_idx)
    bsz = node_max.shape[0]
    nu = ns - r
    slot = np.zeros((bsz, n), dtype=np.int64)
    unm_tok = np.zeros((bsz, nu), dtype=np.int64)
    seg_start = np.zeros((bsz, nd + 1), dtype=np.int64)
    members = np.zeros((bsz, r), dtype=np.int64)
    for b in range(bsz):
        # stable descending: largest first, ties to the lower src position
        order = sorted(range(ns), key=lambda i: (-float(node_max[b, i]), i))
        merged = set(order[:r])
        unm = [i for i in range(ns) if i not in merged]
        for u, i in enumerate(unm):
            unm_tok[b, u] = src[i]
            slot[b, src[i]] = u
        for j in range(nd):
            slot[b, dst[j]] = nu + j
        at = 0
        for j in range(nd):
            seg_start[b, j] = at
            for i in range(ns):  # ascending src position = token position
                if i in merged and int(node_idx[b, i]) == j:
                    members[b, at] = src[i]
                    slot[b, src[i]] = nu + j
                    at += 1
        seg_start[b, nd] = at
        assert at == r
    return dict(slot=slot, unm_tok=unm_tok, seg_start=seg_start,
                members=members)


def merge(x: torch.Tensor, h: int, w: int, p) -> np.ndarray:
    """fp64 merged sequence [B, N-r, C] of x under plan dict p."""
    _, dst = partition(h, w)
    xd = x.detach().cpu().double().numpy()
    bsz = xd.shape[0]
    rows = []
    for b in range(bsz):
        out = [xd[b, t] for t in p["unm_tok"][b]]
        for j, t in enumerate(dst):
            lo, hi = p["seg_start"][b, j], p["seg_start"][b, j + 1]
            acc = xd[b, t].copy()
            for m in p["members"][b, lo:hi]:
                acc = acc + xd[b, m]
            out.append(acc / (1 + hi - lo))
        rows.append(np.stack(out))
    return np.stack(rows)


# ---------------------------------------------------------------------------
# input families (bf16 [BATCH, h*w, WIDTH], fixed seeds)
# ---------------------------------------------------------------------------
def random_input(h: int, w: int, seed: int = 0, c: int = WIDTH):
    g = torch.Generator().manual_seed(1000 + seed + 131 * h + w)
    return torch.randn(BATCH, h * w, c, generator=g).to(torch.bfloat16)


def planted_input(h: int, w: int, seed: int = 0, c: int = WIDTH,
                  noise=2.0 ** -6, target=None):
    """a_i = c_i * b_pi(i) + noise * n_i, c_i in [0.5, 2). Returns (x, pi)
    with pi int64 [BATCH, Ns]. target(b, i, nd) overrides the default
    pi(i) = (7 i + 3 b) % Nd. noise may be a [Ns] tensor."""
    src, dst = partition(h, w)
    ns, nd = len(src), len(dst)
    g = torch.Generator().manual_seed(2000 + seed + 131 * h + w)
    x = torch.randn(BATCH, h * w, c, generator=g)
    x = x.to(torch.bfloat16).float()  # dst rows as the kernel will see them
    pi = torch.empty(BATCH, ns, dtype=torch.int64)
    for b in range(BATCH):
        for i in range(ns):
            pi[b, i] = target(b, i, nd) if target else (7 * i + 3 * b) % nd
    scale = 0.5 + 1.5 * torch.rand(BATCH, ns, generator=g)
    nz = torch.randn(BATCH, ns, c, generator=g)
    nz = nz * torch.as_tensor(noise, dtype=torch.float32).reshape(-1, 1)
    dst_t = torch.from_numpy(dst)
    for b in range(BATCH):
        x[b, torch.from_numpy(src)] = (
            scale[b, :, None] * x[b, dst_t[pi[b]]] + nz[b]
        )
    return x.to(torch.bfloat16), pi
