"""Op entry points: hand-written CDNA4 HIP kernels on GPU, plain PyTorch on CPU.

Policy (no multi-backend dispatch): there are exactly two paths per op —
  * tensors on a HIP device  -> the in-tree gfx950 extension, ALWAYS. If the
    extension is missing on a GPU machine the op raises immediately instead
    of silently falling back to eager PyTorch.
  * tensors on CPU           -> a plain fp32 PyTorch reference used by the
    CPU test suite and as the numerics oracle for the kernels.

The extension is built in-tree (sdwd_amd/ops/_sdwd_hip*.so) by
``python -m sdwd_amd.ops.build`` / ``__graft_entry__.build()`` so the .so
travels with the repo snapshot to GPU boxes.
"""
from __future__ import annotations

import math
import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_ext():
    """Load the in-tree HIP extension (once)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        import importlib

        mod = importlib.import_module("sdwd_amd.ops._sdwd_hip")
        _EXT = mod
    except ImportError:
        # the .so is loaded as an extension module next to this file
        import glob
        import importlib.util

        here = os.path.dirname(os.path.abspath(__file__))
        cands = sorted(glob.glob(os.path.join(here, "_sdwd_hip*.so")))
        if not cands:
            _EXT_ERR = (
                "sdwd_amd HIP extension not built; run "
                "`python -m sdwd_amd.ops.build` (gfx950)"
            )
            return None
        spec = importlib.util.spec_from_file_location("sdwd_amd_hip", cands[0])
        mod = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(mod)
            _EXT = mod
        except Exception as exc:  # pragma: no cover
            _EXT_ERR = f"failed to load {cands[0]}: {exc}"
            return None
    return _EXT


def ext():
    """The HIP extension module; raises loudly when absent on a GPU box."""
    mod = _load_ext()
    if mod is None:
        raise RuntimeError(
            f"sdwd_amd: GPU tensor hit an op but the HIP extension is not "
            f"loaded ({_EXT_ERR}). No eager fallback on GPU by design."
        )
    return mod


def have_ext() -> bool:
    return _load_ext() is not None


# ---------------------------------------------------------------------------
# fused GroupNorm (+ optional SiLU)
# ---------------------------------------------------------------------------
def group_norm_silu(
    x: torch.Tensor,
    weight: torch.Tensor,
    bias: torch.Tensor,
    groups: int = 32,
    eps: float = 1e-5,
    silu: bool = True,
) -> torch.Tensor:
    """GroupNorm over NCHW with the SiLU fused into the normalisation pass.

    The UNet/VAE hot path calls this before every conv; on
    gfx950 it is one kernel: a two-pass (stats, then normalise+activate)
    HBM-bound sweep with ushort8-vectorised bf16 loads.
    """
    if x.is_cuda:
        # keep channels_last only when the NHWC kernel accepts the shape;
        # otherwise force plain NCHW contiguity (mirrors ext.hip dispatch)
        c = x.shape[1]
        nhwc_ok = (
            x.is_contiguous(memory_format=torch.channels_last)
            and x.dtype == torch.bfloat16
            and c % 8 == 0
            and 8 < c <= 3072
        )
        if not nhwc_ok and not x.is_contiguous():
            x = x.contiguous()
        if nhwc_ok and _gn_tile_eligible(x):
            # stats come from the producer's side-channel (conv epilogue,
            # add_gn): the full-tensor stats read is skipped entirely. A
            # tensor nobody produced partials for gets them here, once,
            # and keeps them for its later consumers.
            meta = _valid_gn_partials(x)
            if meta is None:
                gnp = ext().gn_tile_stats(x)
                _attach_gn_partials(x, gnp)
                meta = (gnp, (x.shape[2] * x.shape[3]) // 128)
            return ext().group_norm_silu_pre(
                x, weight, bias, groups, eps, silu, meta[0], meta[1]
            )
        return ext().group_norm_silu(x, weight, bias, groups, eps, silu)
    out = F.group_norm(x.float(), groups, weight.float(), bias.float(), eps)
    if silu:
        out = F.silu(out)
    return out.to(x.dtype)


def group_norm(x, weight, bias, groups: int = 32, eps: float = 1e-5):
    return group_norm_silu(x, weight, bias, groups, eps, silu=False)


# ---------------------------------------------------------------------------
# LayerNorm (transformer blocks)
# ---------------------------------------------------------------------------
def layer_norm(
    x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5
) -> torch.Tensor:
    if x.is_cuda:
        return ext().layer_norm(x.contiguous(), weight, bias, eps)
    return F.layer_norm(
        x.float(), (x.shape[-1],), weight.float(), bias.float(), eps
    ).to(x.dtype)


def add_layer_norm(x, res, weight, bias, eps: float = 1e-5, gather=None):
    """(x + res, LayerNorm(x + res)) in one kernel (transformer residuals).

    gather (token merging): an int32 [B, N] table, plan.slot. res is then
    the merged sequence [B, M, D] and row t of x adds res[b, gather[b, t]]:
    the unmerge folded into the add, so the unmerged tensor never exists."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 \
            and x.shape[-1] <= 1536:
        if gather is not None:
            out = ext().add_layer_norm_gather(
                x, res, weight, bias, eps, gather.contiguous()
            )
        else:
            out = ext().add_layer_norm(x, res, weight, bias, eps)
        return out[0], out[1]
    if gather is not None:
        res = _tome_gather_rows(res, gather)
    s = (x.float() + res.float()).to(x.dtype)
    return s, layer_norm(s, weight, bias, eps)


# ---------------------------------------------------------------------------
# token merging (ToMe) for the level-0 self-attention: 2x2 partition, cosine
# match, plan, merge, unmerge. Kernels in ops/hip/tome.hip; every op has a
# plain torch path (CPU route, oracle, and the composed GPU route for widths
# and dtypes without a kernel). docs/kernels.md has the definition.
# ---------------------------------------------------------------------------
_TOME_PARTITIONS: dict = {}
_TOME_NORM_FLOOR = 2.0 ** -80


def tome_merge_count(h: int, w: int, ratio: float) -> int:
    """r = min(Ns, int(N * ratio)): src tokens merged away per batch row."""
    n = int(h) * int(w)
    nd = (int(h) // 2) * (int(w) // 2)
    if nd == 0:  # a one-token-wide grid has no dst to merge into
        return 0
    return max(0, min(n - nd, int(n * float(ratio))))


def _tome_partition_all(h: int, w: int, device):
    """(src_tok, dst_tok, inv): the int32 tables and the int64 inverse of the
    permutation cat(src_tok, dst_tok), cached per (h, w, device)."""
    h, w = int(h), int(w)
    if h < 2 or w < 2:
        raise ValueError(f"tome_partition: needs h, w >= 2 (got {h}x{w})")
    device = torch.device(device)
    key = (h, w, device)
    hit = _TOME_PARTITIONS.get(key)
    if hit is None:
        yy = torch.arange(h)[:, None].expand(h, w)
        xx = torch.arange(w)[None, :].expand(h, w)
        is_dst = (
            (yy % 2 == 0) & (xx % 2 == 0)
            & (yy < 2 * (h // 2)) & (xx < 2 * (w // 2))
        ).reshape(-1)
        tok = torch.arange(h * w)
        src, dst = tok[~is_dst], tok[is_dst]
        inv = torch.empty(h * w, dtype=torch.int64)
        inv[torch.cat([src, dst])] = tok
        hit = (
            src.to(torch.int32).to(device),
            dst.to(torch.int32).to(device),
            inv.to(device),
        )
        _TOME_PARTITIONS[key] = hit
    return hit


def tome_partition(h: int, w: int, device="cpu"):
    """int32 tables (src_tok [Ns], dst_tok [Nd]) of the 2x2 partition of an
    h x w token grid, ascending, cached per (h, w, device). Token (y, x) is
    dst iff y and x are even and inside the 2*(h//2) x 2*(w//2) region."""
    src, dst, _ = _tome_partition_all(h, w, device)
    return src, dst


def tome_match_supported(x: torch.Tensor) -> bool:
    """True when tome_match runs tome_match_bf16_kernel on x: a bf16 GPU
    tensor [B, N, C] of a width with an instantiation (C = 320)."""
    return bool(
        x.is_cuda and x.dim() == 3 and x.dtype == torch.bfloat16
        and ext().tome_match_supported_width(x.shape[-1])
    )


def tome_match(x: torch.Tensor, h: int, w: int):
    """(node_max fp32 [B, Ns], node_idx int32 [B, Ns]): for every src token
    of x [B, h*w, C] its largest cosine score over the dst tokens of the same
    batch row and the lowest dst index attaining it. 1/|v| is
    rsqrt(max(sum v^2, 2^-80)).

    GPU, tome_match_supported(x): tome_match_bf16_kernel, scores never
    materialised. Other widths / dtypes on the GPU, and the CPU: fp32 bmm +
    max (the CPU path is the oracle of the kernel)."""
    if x.dim() != 3 or x.shape[1] != int(h) * int(w):
        raise ValueError("tome_match: x must be [B, h*w, C]")
    src, dst, _ = _tome_partition_all(h, w, x.device)
    if tome_match_supported(x):
        out = ext().tome_match(x.contiguous(), src, dst)
        return out[0], out[1]
    xf = x.float()
    a = xf[:, src.long()]
    b = xf[:, dst.long()]
    rna = torch.rsqrt((a * a).sum(-1).clamp_min(_TOME_NORM_FLOOR))
    rnb = torch.rsqrt((b * b).sum(-1).clamp_min(_TOME_NORM_FLOOR))
    score = torch.bmm(a, b.transpose(1, 2)) * rnb[:, None, :]
    mx = score.max(dim=-1).values
    nd = score.shape[-1]
    ar = torch.arange(nd, device=x.device)
    idx = torch.where(score == mx[..., None], ar, nd).min(dim=-1).values
    idx = idx.clamp_max(nd - 1)  # a NaN row matches nothing
    return mx * rna, idx.to(torch.int32)


class TomePlan:
    """The integer side of one merge: int32 tensors on the data's device.
    slot [B, N]: row of the merged sequence that token t reads back;
    unm_tok [B, Ns-r]: unmerged src tokens, ascending; seg_start [B, Nd+1]
    and members [B, r]: CSR of every dst's merged src tokens, ascending
    token position inside a segment; dst_tok [Nd]."""

    __slots__ = ("h", "w", "r", "slot", "unm_tok", "seg_start", "members",
                 "dst_tok")

    def __init__(self, h, w, r, slot, unm_tok, seg_start, members, dst_tok):
        self.h, self.w, self.r = h, w, r
        self.slot, self.unm_tok = slot, unm_tok
        self.seg_start, self.members, self.dst_tok = seg_start, members, dst_tok

    @property
    def tokens(self) -> int:
        return self.h * self.w

    @property
    def merged_tokens(self) -> int:
        return self.h * self.w - self.r

    def tensors(self):
        return (self.slot, self.unm_tok, self.seg_start, self.members)


def tome_plan(node_max, node_idx, h: int, w: int, r: int) -> TomePlan:
    """Select the r src tokens with the largest node_max (ties to the lower
    src position) and lay out the merge. Torch integer ops with static
    shapes on node_max's device, the same on CPU and GPU: two stable sorts,
    a cumsum, a searchsorted and scatters to unique (or discarded) targets.
    No host sync, no atomics, so it captures into a hipGraph."""
    src, dst, inv = _tome_partition_all(h, w, node_max.device)
    ns, nd = src.numel(), dst.numel()
    bsz = node_max.shape[0]
    r = int(r)
    if tuple(node_max.shape) != (bsz, ns) or tuple(node_idx.shape) != (bsz, ns):
        raise ValueError(f"tome_plan: node_max/node_idx must be [B, {ns}]")
    if not 0 <= r <= ns:
        raise ValueError(f"tome_plan: r must lie in [0, {ns}] (got {r})")
    dev = node_max.device
    nu = ns - r
    pos = torch.arange(ns, device=dev)
    order = torch.sort(
        node_max.float(), dim=1, descending=True, stable=True
    ).indices
    rank = torch.empty_like(order)
    rank.scatter_(1, order, pos[None].expand(bsz, ns))
    merged = rank < r                                     # [B, Ns]
    didx = node_idx.long().clamp(0, nd - 1)
    # unmerged src tokens keep their order: slot = rank among the unmerged
    urank = torch.cumsum((~merged).to(torch.int64), dim=1) - 1
    slot_src = torch.where(merged, nu + didx, urank)
    slot_dst = (nu + torch.arange(nd, device=dev))[None].expand(bsz, nd)
    slot = torch.cat([slot_src, slot_dst], dim=1)[:, inv]
    # unm_tok: every unmerged src writes its own cell; the merged ones all
    # land in a spare cell that is cut off
    buf = torch.empty(bsz, nu + 1, dtype=torch.int64, device=dev)
    buf.scatter_(
        1, torch.where(merged, nu, urank), src.long()[None].expand(bsz, ns)
    )
    unm_tok = buf[:, :nu]
    # CSR of members per dst: stable sort of dst-or-sentinel keys in token
    # order, segment starts by binary search
    keys = torch.where(merged, didx, nd)
    skeys, perm = torch.sort(keys, dim=1, stable=True)
    members = src.long()[perm[:, :r]]
    bounds = torch.arange(nd + 1, device=dev)[None].expand(bsz, nd + 1)
    seg_start = torch.searchsorted(skeys.contiguous(), bounds.contiguous())
    i32 = torch.int32
    return TomePlan(
        int(h), int(w), r, slot.to(i32).contiguous(),
        unm_tok.to(i32).contiguous(), seg_start.to(i32).contiguous(),
        members.to(i32).contiguous(), dst,
    )


def _tome_native_rows(x: torch.Tensor) -> bool:
    return bool(
        x.is_cuda and x.dim() == 3 and x.dtype == torch.bfloat16
        and x.shape[-1] % 8 == 0
    )


def _tome_gather_rows(y: torch.Tensor, slot: torch.Tensor) -> torch.Tensor:
    idx = slot.long()[..., None].expand(-1, -1, y.shape[-1])
    return torch.gather(y, 1, idx)


def tome_merge(x: torch.Tensor, plan: TomePlan, native: bool = True):
    """x [B, N, C] -> [B, N-r, C]: the unmerged src tokens in ascending
    position, then the dst tokens, each (dst + its members) / (1 + count),
    summed in fp32 dst first then members in CSR order, one true division,
    one rounding to x's dtype.

    GPU bf16 with C % 8 == 0: tome_merge_bf16_kernel. Otherwise (and with
    native=False, the composed route for comparisons) the same arithmetic
    in torch, one step per member rank; its loop bound is the largest
    segment, read on the host, so that route does not capture."""
    bsz, n, c = x.shape
    if n != plan.tokens:
        raise ValueError("tome_merge: x and plan disagree on the token count")
    if native and _tome_native_rows(x):
        return ext().tome_merge(
            x.contiguous(), plan.dst_tok, plan.unm_tok, plan.seg_start,
            plan.members,
        )
    seg = plan.seg_start.long()
    start, stop = seg[:, :-1], seg[:, 1:]
    count = stop - start
    members = plan.members.long()
    acc = x[:, plan.dst_tok.long()].float()
    depth = int(count.max()) if plan.r > 0 else 0
    for k in range(depth):
        live = (k < count)
        at = (start + k).clamp_max(max(plan.r - 1, 0))
        tok = torch.gather(members, 1, at)
        rows = _tome_gather_rows(x, tok).float()
        acc = torch.where(live[..., None], acc + rows, acc)
    dstrows = (acc / (1 + count).float()[..., None]).to(x.dtype)
    unm = _tome_gather_rows(x, plan.unm_tok)
    return torch.cat([unm, dstrows], dim=1)


def tome_unmerge(y: torch.Tensor, plan: TomePlan, native: bool = True):
    """y [B, N-r, C] -> [B, N, C]: every original token gets the row of its
    slot. GPU bf16, C % 8 == 0: tome_unmerge_bf16_kernel; else a gather."""
    if y.shape[1] != plan.merged_tokens:
        raise ValueError("tome_unmerge: y and plan disagree on the row count")
    if native and _tome_native_rows(y):
        return ext().tome_unmerge(y.contiguous(), plan.slot)
    return _tome_gather_rows(y, plan.slot)


# ---------------------------------------------------------------------------
# attention (flash-style, fused softmax(QK^T/sqrt(d))·V)
# ---------------------------------------------------------------------------
# flash kernel variants -> the extension's `force` argument; SDWD_ATTN keeps
# its historical spellings (v2, v3all)
_ATTN_FORCE = {"auto": 0, "v2": 2, "v3": 3}
_ATTN_ENV = {"v2": 2, "v3all": 3}
_ATTN_ENV_FORCE: Optional[int] = None


def _attn_force(variant: Optional[str]) -> int:
    """None -> SDWD_ATTN (read once; v2 / v3all, anything else is auto); an
    explicit variant always wins and must be one of auto/v2/v3."""
    global _ATTN_ENV_FORCE
    if variant is None:
        if _ATTN_ENV_FORCE is None:
            _ATTN_ENV_FORCE = _ATTN_ENV.get(
                os.environ.get("SDWD_ATTN", ""), 0
            )
        return _ATTN_ENV_FORCE
    if variant not in _ATTN_FORCE:
        raise ValueError(
            f"attention: unknown variant {variant!r} "
            f"(expected one of {sorted(_ATTN_FORCE)})"
        )
    return _ATTN_FORCE[variant]


def attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
    variant: Optional[str] = None,
) -> torch.Tensor:
    """q,k,v: [B, H, S, D] -> [B, H, Sq, D]. bf16 in/out on GPU, fp32 accum.

    GPU path: hand-written MFMA flash-forward kernel (ops/hip/attention.hip),
    online softmax, D padded to a multiple of 16 in-kernel. variant picks
    the kernel: "auto" is the measured dispatch (ext().attention_plan), "v2"
    / "v3" force one flash kernel and raise on a head dim that has none;
    None follows SDWD_ATTN.
    CPU path: explicit fp32 reference (the numerics oracle).
    """
    force = _attn_force(variant)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        # SDWD_ATTN only steers calls that a flash kernel can take (an A/B
        # run still composes the VAE's D=512); an explicit variant on any
        # other call is an error in the extension
        if variant is None and not (
            ext().flash_supported(q.shape[-1])
            and q.dtype == torch.bfloat16
            and q.stride(-1) == k.stride(-1) == v.stride(-1) == 1
        ):
            force = 0
        return ext().attention_fwd(q, k, v, scale, force)
    qf, kf, vf = q.float(), k.float(), v.float()
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    return torch.matmul(p, vf).to(q.dtype)


def attention_bshd(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
    variant: Optional[str] = None,
) -> torch.Tensor:
    """q,k,v: [B, S, H, D] (natural projection layout) -> [B, Sq, H, D].

    GPU: strided flash kernel, zero transpose/pad copies. CPU (or an
    unsupported head dim): permuted reference path. variant as in
    attention().
    """
    force = _attn_force(variant)
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda:
        mod = ext()
        d = q.shape[-1]
        if mod.flash_supported(d):
            return mod.attention_fwd_bshd(q, k, v, scale, force)
    out = attention(
        q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3),
        scale, variant,
    )
    return out.permute(0, 2, 1, 3)


# ---------------------------------------------------------------------------
# Hypertile: self-attention inside rectangular windows of the token grid
# ---------------------------------------------------------------------------
def _window_extent(n: int, least: int) -> int:
    """The smallest divisor of n that is >= least (n itself at the latest)."""
    for t in range(max(1, least), n + 1):
        if n % t == 0:
            return t
    return n


def hypertile_windows(
    width: int, height: int, h: int, w: int, depth: int, max_tile: int = 256
) -> Tuple[int, int]:
    """(nh, nw): how many windows a self-attention layer's h x w token grid
    is cut into, for a pass of width x height pixels. depth is the rank of
    the layer's resolution among the UNet's transformer stages (finest 0).

    The host's rule at swap size 1, deterministic: P = the largest power of
    two dividing gcd(width, height); T = min(max_tile, P); L = max(128, T)
    // 8; along each axis the window is the smallest divisor of the extent
    that is >= min(L * 2**depth, extent). (1, 1) means the layer is left
    alone; the max_depth cut-off is the caller's (UNetModel.set_hypertile).
    """
    for name, val in (("width", width), ("height", height), ("h", h), ("w", w)):
        if isinstance(val, bool) or not isinstance(val, int) or val < 1:
            raise ValueError(f"hypertile_windows: {name} must be a positive "
                             f"integer (got {val!r})")
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 0:
        raise ValueError(f"hypertile_windows: depth must be an integer >= 0 "
                         f"(got {depth!r})")
    if (isinstance(max_tile, bool) or not isinstance(max_tile, int)
            or max_tile < 0):
        raise ValueError(f"hypertile_windows: max_tile must be an integer "
                         f">= 0 (got {max_tile!r})")
    g = math.gcd(width, height)
    p = g & -g
    least = max(128, min(max_tile, p)) // 8 * 2 ** depth
    th = _window_extent(h, min(least, h))
    tw = _window_extent(w, min(least, w))
    return h // th, w // tw


def _window_args(name, q, k, v, grid, window):
    """Validated (B, S, H, D, gh, gw, th, tw) of a windowed attention call."""
    for n, t in (("q", q), ("k", k), ("v", v)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: {n} must be a [B, S, H, D] tensor")
    if tuple(k.shape) != tuple(q.shape) or tuple(v.shape) != tuple(q.shape):
        raise ValueError(f"{name}: q, k and v must have one shape (self-"
                         f"attention); got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)}")
    if k.device != q.device or v.device != q.device:
        raise ValueError(f"{name}: q, k and v must share a device")
    pairs = []
    for n, pair in (("grid", grid), ("window", window)):
        try:
            a, b = pair
        except (TypeError, ValueError):
            raise ValueError(f"{name}: {n} must be a pair of integers "
                             f"(got {pair!r})") from None
        for x in (a, b):
            if isinstance(x, bool) or not isinstance(x, int) or x < 1:
                raise ValueError(f"{name}: {n} must hold positive integers "
                                 f"(got {pair!r})")
        pairs.append((a, b))
    (gh, gw), (th, tw) = pairs
    B, S, H, D = q.shape
    if B < 1 or H < 1 or D < 1:
        raise ValueError(f"{name}: q, k and v must be non-empty")
    if gh * gw != S:
        raise ValueError(f"{name}: grid {gh}x{gw} does not match the token "
                         f"count {S}")
    if gh % th or gw % tw:
        raise ValueError(f"{name}: window {th}x{tw} does not divide the "
                         f"grid {gh}x{gw}")
    return B, S, H, D, gh, gw, th, tw


def window_split(x: torch.Tensor, grid, window) -> torch.Tensor:
    """[B, gh*gw, ...] -> [B*nh*nw, th*tw, ...]: the windows of the token
    grid as batch rows (a copy), window (i, j) of batch b at row
    (b*nh + i)*nw + j. The host's `b (nh h nw w) c -> (b nh nw) (h w) c`."""
    (gh, gw), (th, tw) = grid, window
    nh, nw = gh // th, gw // tw
    b, rest = x.shape[0], tuple(x.shape[2:])
    nd = len(rest)
    x = x.reshape(b, nh, th, nw, tw, *rest)
    x = x.permute(0, 1, 3, 2, 4, *range(5, 5 + nd))
    return x.reshape(b * nh * nw, th * tw, *rest)


def window_merge(x: torch.Tensor, grid, window) -> torch.Tensor:
    """The inverse of window_split: [B*nh*nw, th*tw, ...] -> [B, gh*gw, ...]."""
    (gh, gw), (th, tw) = grid, window
    nh, nw = gh // th, gw // tw
    b, rest = x.shape[0] // (nh * nw), tuple(x.shape[2:])
    nd = len(rest)
    x = x.reshape(b, nh, nw, th, tw, *rest)
    x = x.permute(0, 1, 3, 2, 4, *range(5, 5 + nd))
    return x.reshape(b, gh * gw, *rest)


def attention_window_supported(q, k, v) -> bool:
    """True when attention_window_bshd runs the windowed kernel on these
    tensors: on the GPU, bf16, a head dim with a flash kernel, unit stride
    in D and 16-byte-aligned rows (what the fused QKV slices have)."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda
            and q.dtype == k.dtype == v.dtype == torch.bfloat16
            and ext().flash_supported(q.shape[-1])):
        return False
    for t in (q, k, v):
        if t.stride(-1) != 1 or t.data_ptr() % 16:
            return False
        if any(t.shape[i] != 1 and t.stride(i) % 8 for i in range(3)):
            return False
    return True


def attention_window_bshd(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    grid,
    window,
    scale: Optional[float] = None,
    native: bool = True,
) -> torch.Tensor:
    """Self-attention inside the windows of a token grid (Hypertile).

    q, k, v: [B, gh*gw, H, D] (strided views as attention_bshd takes), grid
    = (gh, gw), window = (th, tw) with th | gh and tw | gw. Token (Y, X)
    attends to the th*tw tokens of window (Y // th, X // tw); the output is
    [B, gh*gw, H, D] in the original token order.

    GPU, bf16, flash head dim: flash_fwd_bf16_v3's WIN mode reads q/k/v and
    writes the output in place, no rearranged copies. native=False (A/B
    timing, comparison tests) and every other GPU case (D=512, fp32): the
    windows are materialised (window_split) and go through attention_bshd.
    CPU: the same rearrangement on the fp32 reference (the oracle).
    window == grid returns exactly what attention_bshd returns.
    """
    name = "attention_window"
    B, S, H, D, gh, gw, th, tw = _window_args(name, q, k, v, grid, window)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if (th, tw) == (gh, gw):
        return attention_bshd(q, k, v, scale)
    if q.is_cuda and native and attention_window_supported(q, k, v):
        return ext().attention_window_bshd(q, k, v, gh, gw, th, tw, scale)
    g, w = (gh, gw), (th, tw)
    out = attention_bshd(
        window_split(q, g, w), window_split(k, g, w), window_split(v, g, w),
        scale,
    )
    return window_merge(out, g, w)


# ---------------------------------------------------------------------------
# multi-context attention blend (regional prompting, decoupled cross-attn)
# ---------------------------------------------------------------------------
def attention_blend_supported(q, k, v) -> bool:
    """True when attention_blend_bshd runs its kernel on these tensors: on
    the GPU, bf16, a head dim with a flash kernel, unit stride in D."""
    return bool(
        q.is_cuda and k.is_cuda and v.is_cuda
        and q.dtype == k.dtype == v.dtype == torch.bfloat16
        and ext().flash_supported(q.shape[-1])
        and q.stride(-1) == k.stride(-1) == v.stride(-1) == 1
    )


def _blend_table(name, table, shape, lo, hi, device):
    """A small integer table for the blend kernel as int32 on `device`. A
    device int32 tensor is taken as it is (the caller validated and cached
    it); anything else is validated on the host, so no device sync."""
    if (torch.is_tensor(table) and table.device.type != "cpu"
            and table.dtype == torch.int32):
        if tuple(table.shape) != shape:
            raise ValueError(
                f"attention_blend: {name} has shape {tuple(table.shape)}, "
                f"expected {shape}"
            )
        if table.device != device:
            raise ValueError(
                f"attention_blend: {name} is on {table.device}, q on {device}"
            )
        return table.contiguous()
    if torch.is_tensor(table):
        if table.device.type != "cpu":
            raise ValueError(
                f"attention_blend: a device {name} must be int32 "
                f"(got {table.dtype})"
            )
        if table.dtype.is_floating_point or table.dtype == torch.bool:
            raise ValueError(f"attention_blend: {name} must hold integers")
        t = table.to(torch.int64)
    else:
        try:
            t = torch.tensor(table, dtype=torch.int64)
        except (TypeError, ValueError, RuntimeError) as exc:
            raise ValueError(
                f"attention_blend: {name} is not an integer table: {exc}"
            ) from None
    if tuple(t.shape) != shape:
        raise ValueError(
            f"attention_blend: {name} has shape {tuple(t.shape)}, "
            f"expected {shape}"
        )
    if t.numel() and (int(t.min()) < lo or int(t.max()) > hi):
        raise ValueError(
            f"attention_blend: {name} entries must lie in [{lo}, {hi}] "
            f"(got {int(t.min())}..{int(t.max())})"
        )
    return t.to(torch.int32).contiguous().to(device)


def attention_blend_bshd(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    w: torch.Tensor,
    kv_index,
    kv_len=None,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """Weighted sum of attentions that share Q, in one kernel:

        out[b,s,h,:] = sum_c w[b,c,s] * softmax(scale * q[b,s,h] K_c^T) V_c

    with K_c, V_c = k[kv_index[b][c]], v[kv_index[b][c]] cut to their first
    kv_len[kv_index[b][c]] keys. q [B,Sq,H,D]; k, v [Bk,Sk,H,D] (strided
    views with unit stride in D, as attention_bshd takes); w fp32 [B,C,Sq]
    or [1,C,Sq]; kv_index [B,C] and kv_len [Bk] (None: all Sk keys) are CPU
    integer tensors or lists, validated here without a device sync, or
    device int32 tensors, taken unvalidated so a caller can cache them.

    GPU path: flash_blend_bf16_kernel (ops/hip/attention.hip): per-context
    online softmax, fp32 blend in registers, one bf16 rounding. bf16 and a
    head dim with a flash kernel only; anything else raises, the blend is
    never composed from separate attentions.
    CPU path: plain fp32 reference (the numerics oracle).
    """
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4:
            raise ValueError(f"attention_blend: {name} must be [B, S, H, D]")
    B, Sq, H, D = q.shape
    Bk, Sk = k.shape[0], k.shape[1]
    if tuple(k.shape) != tuple(v.shape):
        raise ValueError("attention_blend: k and v shapes differ")
    if Bk < 1 or Sk < 1 or B < 1 or Sq < 1:
        raise ValueError("attention_blend: q, k and v must be non-empty")
    if tuple(k.shape[2:]) != (H, D):
        raise ValueError(
            f"attention_blend: k has heads/dim {tuple(k.shape[2:])}, "
            f"q has {(H, D)}"
        )
    if not torch.is_tensor(w) or w.dim() != 3 or w.dtype != torch.float32:
        raise ValueError("attention_blend: w must be an fp32 [B, C, Sq] tensor")
    C = w.shape[1]
    if C < 1:
        raise ValueError("attention_blend: w needs at least one context (C >= 1)")
    if w.shape[0] not in (1, B) or w.shape[2] != Sq:
        raise ValueError(
            f"attention_blend: w has shape {tuple(w.shape)}, expected "
            f"[{B} or 1, C, {Sq}]"
        )
    if w.device != q.device or k.device != q.device or v.device != q.device:
        raise ValueError("attention_blend: q, k, v and w must share a device")
    idx = _blend_table("kv_index", kv_index, (B, C), 0, Bk - 1, q.device)
    lens = None
    if kv_len is not None:
        lens = _blend_table("kv_len", kv_len, (Bk,), 1, Sk, q.device)
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    if q.is_cuda:
        if w.stride(2) != 1:
            w = w.contiguous()
        return ext().attention_blend_bshd(q, k, v, w, idx, lens, scale)
    idx = idx.tolist()
    lens = [Sk] * Bk if lens is None else lens.tolist()
    qf = q.float().permute(0, 2, 1, 3)                    # [B, H, Sq, D]
    out = torch.zeros(B, H, Sq, D, dtype=torch.float32)
    for b in range(B):
        wb = w[b if w.shape[0] > 1 else 0]
        for c in range(C):
            row = idx[b][c]
            n = lens[row]
            kf = k[row, :n].float().permute(1, 0, 2)      # [H, n, D]
            vf = v[row, :n].float().permute(1, 0, 2)
            p = torch.softmax(qf[b] @ kf.transpose(-1, -2) * scale, dim=-1)
            out[b] += wb[c][None, :, None] * (p @ vf)
    return out.permute(0, 2, 1, 3).to(q.dtype)


# ---------------------------------------------------------------------------
# GEGLU activation: x, gate = split(h); x * gelu(gate)
# ---------------------------------------------------------------------------
def geglu(h: torch.Tensor) -> torch.Tensor:
    if h.is_cuda:
        return ext().geglu(h.contiguous())
    x, gate = h.float().chunk(2, dim=-1)
    return (x * F.gelu(gate)).to(h.dtype)


def silu(x: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        return ext().silu(x.contiguous())
    return F.silu(x.float()).to(x.dtype)


# ---------------------------------------------------------------------------
# sampler-step elementwise kernels (denoise loop, hipGraph-capturable)
# ---------------------------------------------------------------------------
def euler_step(
    x: torch.Tensor, denoised: torch.Tensor, sigma: float, sigma_next: float
) -> torch.Tensor:
    """x + (x - denoised)/sigma * (sigma_next - sigma), one fused kernel."""
    if x.is_cuda:
        return ext().euler_step(
            x.contiguous(), denoised.contiguous(), sigma, sigma_next
        )
    d = (x.float() - denoised.float()) / sigma
    return (x.float() + d * (sigma_next - sigma)).to(x.dtype)


def add_noise(
    x: torch.Tensor, noise: torch.Tensor, a: float, b: float
) -> torch.Tensor:
    """a*x + b*noise in one pass (ancestral samplers, img2img noising)."""
    if x.is_cuda:
        return ext().axpby(x.contiguous(), noise.contiguous(), a, b)
    return (a * x.float() + b * noise.float()).to(x.dtype)


def lincomb(x: torch.Tensor, y: torch.Tensor, a: float, b: float):
    """a*x + b*y, fp32 math, one kernel (sampler updates, CFG combine)."""
    return add_noise(x, y, a, b)


def scale(x: torch.Tensor, c: float) -> torch.Tensor:
    """c*x in one kernel (sampler input scaling)."""
    if x.is_cuda:
        xc = x.contiguous()
        return ext().axpby(xc, xc, c, 0.0)
    return (c * x.float()).to(x.dtype)


# ---------------------------------------------------------------------------
# counter-based noise: Philox4x32-10 + Box-Muller (the "NV" random source)
# ---------------------------------------------------------------------------
# Element j of draw `offset` of the generator `seed`:
#   counter (offset & M32, offset >> 32, j, 0), key (seed & M32, seed >> 32)
#   (x0, x1, _, _) = philox4x32_10(counter, key)
#   u = float(x0) * 2^-32 + 2^-33          (fp32, in (0, 1])
#   v = float(x1) * 2pi*2^-32 + 2pi*2^-33  (fp32, in (0, 2pi])
#   r = sqrtf(-2 logf(u)) * sinf(v)
# One normal per counter, by definition of that source (docs/usage.md).
_M32 = 0xFFFFFFFF
_PHILOX_M0 = 0xD2511F53
_PHILOX_M1 = 0xCD9E8D57
_PHILOX_W0 = 0x9E3779B9
_PHILOX_W1 = 0xBB67AE85
_TWO_PI = 2.0 * math.pi


def _mulhilo32(m: int, c: torch.Tensor):
    """(hi, lo) words of m*c for a 32-bit constant m and int64 c < 2^32,
    without leaving int64: c is split into 16-bit halves."""
    a = m * (c & 0xFFFF)           # < 2^48
    b = m * (c >> 16)              # < 2^48
    hi = ((a >> 16) + b) >> 16
    lo = (a + ((b & 0xFFFF) << 16)) & _M32
    return hi, lo


def _philox_rounds(c0, c1, c2, c3, k0, k1):
    for _ in range(10):
        h0, l0 = _mulhilo32(_PHILOX_M0, c0)
        h1, l1 = _mulhilo32(_PHILOX_M1, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0 = (k0 + _PHILOX_W0) & _M32
        k1 = (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def _uint32_table(name: str, t, cols: int) -> torch.Tensor:
    t = torch.as_tensor(t)
    if t.dtype != torch.int64 or t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"philox4x32: {name} must be an int64 [N, {cols}]")
    return t


def philox4x32(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Philox4x32-10 at raw counters [N,4] and keys [N,2] -> words [N,4];
    int64 tensors that hold uint32 values. Exists so the core can be pinned
    bit for bit; GPU: philox4x32_kernel (ops/hip/rng.hip), CPU: int64 torch
    ops."""
    counter = _uint32_table("counter", counter, 4)
    key = _uint32_table("key", key, 2)
    if counter.shape[0] != key.shape[0] or counter.device != key.device:
        raise ValueError("philox4x32: counter and key must pair up, [N,4]/[N,2]")
    if counter.is_cuda:
        return ext().philox4x32(counter.contiguous(), key.contiguous())
    c = counter & _M32
    k = key & _M32
    return torch.stack(
        _philox_rounds(c[:, 0], c[:, 1], c[:, 2], c[:, 3], k[:, 0], k[:, 1]),
        dim=1,
    )


def _philox_seeds(seeds, device) -> torch.Tensor:
    """Per-image generator seeds as an int64 [B] table on `device` (the bit
    pattern of the uint64 seed). A device int64 tensor is taken as it is so
    a caller can upload it once; host seeds are validated here."""
    device = torch.device(device)
    if torch.is_tensor(seeds) and seeds.device.type != "cpu":
        if seeds.dtype != torch.int64 or seeds.dim() != 1:
            raise ValueError("philox: a device `seeds` must be an int64 [B]")
        if seeds.device != device:
            raise ValueError(
                f"philox: seeds is on {seeds.device}, expected {device}"
            )
        return seeds.contiguous()
    if torch.is_tensor(seeds):
        if seeds.dtype.is_floating_point or seeds.dtype == torch.bool \
                or seeds.dim() != 1:
            raise ValueError("philox: seeds must be a 1-d table of integers")
        vals = seeds.tolist()
    else:
        vals = list(seeds)
    out = []
    for s in vals:
        if isinstance(s, bool) or not isinstance(s, int):
            raise ValueError(f"philox: seeds must be integers (got {s!r})")
        if not 0 <= s < (1 << 64):
            raise ValueError(
                f"philox: seeds must lie in [0, 2^64) (got {s})"
            )
        out.append(s - (1 << 64) if s >= (1 << 63) else s)
    return torch.tensor(out, dtype=torch.int64).to(device)


def _philox_offset(offset) -> int:
    if isinstance(offset, bool) or not isinstance(offset, int) \
            or not 0 <= offset < (1 << 64):
        raise ValueError(
            f"philox: offset must be an integer in [0, 2^64) (got {offset!r})"
        )
    return offset


def _philox_normals_cpu(seeds: torch.Tensor, offset: int, n: int):
    """fp32 normals [B, n] from an int64 [B] seed table."""
    j = torch.arange(n, dtype=torch.int64)[None, :]
    zero = torch.zeros_like(j)
    k0 = (seeds & _M32)[:, None]
    k1 = ((seeds >> 32) & _M32)[:, None]
    x0, x1, _, _ = _philox_rounds(
        zero + (offset & _M32), zero + (offset >> 32), j, zero,
        k0.expand(-1, n), k1.expand(-1, n),
    )
    u = x0.to(torch.float32) * (2.0 ** -32) + (2.0 ** -33)
    v = x1.to(torch.float32) * (_TWO_PI * 2.0 ** -32) + (_TWO_PI * 2.0 ** -33)
    return torch.sqrt(-2.0 * torch.log(u)) * torch.sin(v)


def philox_randn(
    seeds, offset: int, shape, dtype=torch.float32, device="cpu"
) -> torch.Tensor:
    """[B, *shape] normals: row b is draw `offset` of the generator
    seeds[b]; element j (C-order within `shape`) depends on (seed, offset,
    j) alone, so it is the same on every device, shard and batch position.

    seeds: a list or CPU tensor of integers in [0, 2^64), or a device int64
    tensor (two's-complement bit pattern) taken as it is. GPU:
    philox_randn_kernel; CPU: the same definition in torch int64/fp32 ops
    (the numerics oracle)."""
    device = torch.device(device)
    sd = _philox_seeds(seeds, device)
    offset = _philox_offset(offset)
    shape = tuple(int(s) for s in shape)
    n = int(math.prod(shape))
    if not 0 <= n < (1 << 32):
        raise ValueError("philox_randn: a draw holds fewer than 2^32 elements")
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("philox_randn: dtype must be float32 or bfloat16")
    b = sd.shape[0]
    if device.type == "cuda":
        out = ext().philox_randn(
            sd, offset & _M32, offset >> 32, n, dtype == torch.bfloat16
        )
    else:
        out = _philox_normals_cpu(sd, offset, n).to(dtype)
    return out.reshape(b, *shape)


def add_philox_noise(
    x: torch.Tensor, seeds, offset: int, a: float, b: float
) -> torch.Tensor:
    """a*x + b*philox_randn(seeds, offset, x.shape[1:]) in fp32 math, without
    materialising the noise on the GPU (axpby_philox_kernel, one launch).
    x: [B, C, H, W], fp32 or bf16, contiguous or channels_last (the result
    keeps that format; any other layout is made contiguous first). The noise
    index is the logical (c, h, w) position whatever the memory format."""
    if x.dim() != 4:
        raise ValueError("add_philox_noise: x must be [B, C, H, W]")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("add_philox_noise: x must be float32 or bfloat16")
    sd = _philox_seeds(seeds, x.device)
    offset = _philox_offset(offset)
    if sd.shape[0] != x.shape[0]:
        raise ValueError(
            f"add_philox_noise: {sd.shape[0]} seeds for a batch of "
            f"{x.shape[0]}"
        )
    if not (x.is_contiguous()
            or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.contiguous()
    if x.is_cuda:
        return ext().axpby_philox(
            x, sd, offset & _M32, offset >> 32, float(a), float(b)
        )
    n = x[0].numel()
    if n >= (1 << 32):
        raise ValueError("add_philox_noise: an image holds fewer than 2^32 "
                         "elements")
    r = _philox_normals_cpu(sd, offset, n).reshape(x.shape)
    out = torch.empty_like(x)  # keeps x's memory format
    out.copy_(float(a) * x.float() + float(b) * r)
    return out


def _attach_gn_partials(
    y: torch.Tensor, gnp: Optional[torch.Tensor]
) -> None:
    """Ride the conv's per-tile (sum, sumsq) side-channel on the output
    tensor; a downstream GroupNorm consumes it and skips its stats read.
    The _version pin invalidates the cache if y is ever mutated in place."""
    if gnp is not None and gnp.numel() > 0:
        tpi = (y.shape[2] * y.shape[3]) // 128
        y._sdwd_gnp = (gnp, tpi, y._version)


def _gn_tile_eligible(x: torch.Tensor) -> bool:
    """Can x carry the per-tile GroupNorm partials? bf16 channels_last on
    the GPU, C % 8 == 0, and every 128-row tile inside one image."""
    return (
        x.is_cuda
        and x.dim() == 4
        and x.dtype == torch.bfloat16
        and x.shape[1] % 8 == 0
        and x.numel() > 0
        and (x.shape[2] * x.shape[3]) % 128 == 0
        and x.is_contiguous(memory_format=torch.channels_last)
    )


def _valid_gn_partials(x: torch.Tensor):
    """x's (partials, tiles per image, version) side channel, or None when
    it has none or was mutated in place since they were taken."""
    meta = getattr(x, "_sdwd_gnp", None)
    if (
        meta is not None
        and meta[2] == x._version
        and meta[0].shape[-1] == x.shape[1]
    ):
        return meta
    return None


def add_gn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a + b (bit-equal to the ATen add) that also emits the sum's per-tile
    GroupNorm partials in the same pass, so the next GroupNorm skips its
    stats read (the SpatialTransformer exit). Shapes that cannot carry
    partials get a plain add."""
    if (
        _gn_tile_eligible(a)
        and _gn_tile_eligible(b)
        and a.shape == b.shape
    ):
        out, gnp = ext().add_gn(a, b)
        _attach_gn_partials(out, gnp)
        return out
    return a + b


def cat_channels_gn(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Channel-concat that PRESERVES the GroupNorm partials: a cat along C
    concatenates the per-channel partial sums too, so the UNet up-path's
    skip-concat keeps the stats side-channel alive. When exactly one half
    lacks partials they are computed for that half alone (and stay attached
    to it)."""
    out = torch.cat([a, b], dim=1)
    ma = _valid_gn_partials(a)
    mb = _valid_gn_partials(b)
    if (ma is None) != (mb is None):
        miss = a if ma is None else b
        if _gn_tile_eligible(miss):
            gnp = ext().gn_tile_stats(miss)
            _attach_gn_partials(miss, gnp)
            meta = (gnp, (miss.shape[2] * miss.shape[3]) // 128)
            if ma is None:
                ma = meta
            else:
                mb = meta
    if (
        ma is not None
        and mb is not None
        and ma[1] == mb[1]
        and ma[0].shape[0] == mb[0].shape[0]
    ):
        gnp = torch.cat([ma[0], mb[0]], dim=-1)
        out._sdwd_gnp = (gnp, ma[1], out._version)
    return out


# conv3x3 kernel variants -> the extension's `force` argument
_CONV_FORCE = {"auto": 0, "v2": 2, "v4": 4}
_CONV_ENV_FORCE: Optional[int] = None


def _conv_force(variant: Optional[str]) -> int:
    """None -> SDWD_CONV (read once, unknown values mean auto); an explicit
    variant always wins and must be one of auto/v2/v4."""
    global _CONV_ENV_FORCE
    if variant is None:
        if _CONV_ENV_FORCE is None:
            _CONV_ENV_FORCE = _CONV_FORCE.get(
                os.environ.get("SDWD_CONV", ""), 0
            )
        return _CONV_ENV_FORCE
    if variant not in _CONV_FORCE:
        raise ValueError(
            f"conv3x3: unknown variant {variant!r} "
            f"(expected one of {sorted(_CONV_FORCE)})"
        )
    return _CONV_FORCE[variant]


def conv3x3(
    x: torch.Tensor,
    w_prep: torch.Tensor,
    bias: Optional[torch.Tensor],
    residual: Optional[torch.Tensor],
    stride: int = 1,
    chan_bias: Optional[torch.Tensor] = None,
    collect_gn: bool = False,
    variant: Optional[str] = None,
    wrap: Tuple[bool, bool] = (False, False),
) -> torch.Tensor:
    """NHWC implicit-GEMM 3x3 conv (pad 1); bias, an optional residual and
    an optional per-(sample, channel) bias (the ResBlock time-embedding
    projection) all fused into the epilogue. With collect_gn the epilogue
    also emits per-tile GroupNorm partial sums (see _attach_gn_partials).
    variant picks the kernel: "auto" is the measured dispatch
    (ext().conv3x3_plan), "v2" the 128-tile kernel everywhere, "v4" the
    256x256 pipeline on every legal shape; None follows SDWD_CONV.
    wrap = (height, width): the padding on that axis wraps around (seamless
    tiling) instead of reading zeros; it composes with everything above.
    GPU-only entry."""
    y, gnp = ext().conv3x3_nhwc(
        x, w_prep, bias, residual, chan_bias, stride, collect_gn,
        _conv_force(variant), bool(wrap[0]), bool(wrap[1]),
    )
    _attach_gn_partials(y, gnp)
    return y


def conv3x3_small(
    x: torch.Tensor,
    w_prep: torch.Tensor,
    bias: Optional[torch.Tensor],
    stride: int = 1,
    wrap: Tuple[bool, bool] = (False, False),
) -> torch.Tensor:
    """Direct 3x3 conv for tiny Cin (3/4/9: the stem/IO convs) — keeps the
    whole pipeline off MIOpen's fallback solvers. wrap = (height, width)
    selects wrap-around padding per axis. GPU-only entry."""
    return ext().conv3x3_small(
        x, w_prep, bias, stride, bool(wrap[0]), bool(wrap[1])
    )


def conv3x3_small_supported(cin: int, cout: int) -> bool:
    # LDS weight cache (9*Cin*Cout bf16) must fit the 160 KiB CU budget
    return (
        int(cin) in (3, 4, 9)
        and cout % 8 == 0
        and cout <= 1536
        and 9 * int(cin) * int(cout) * 2 <= 160 * 1024
    )


def fold_ups2x_weight(
    w_prep: torch.Tensor, out: Optional[torch.Tensor] = None
) -> torch.Tensor:
    """[Cout,3,3,Cin] -> [4,Cout,2,2,Cin]: the 3x3 weights folded for a conv
    over a nearest-2x upsample. Output pixel (2i+a, 2j+b) sees source rows
    i-1+a+r, r in {0,1}: phase a=0 weighs them w[0], w[1]+w[2]; a=1 weighs
    them w[0]+w[1], w[2]; columns alike with b, s, kx. Entry p = 2a+b is
    that phase's 2x2 kernel. The sums are formed in fp32 (fp64 for fp64
    input), rows first, in a fixed order, and rounded once to w_prep's
    dtype; `out` is refilled in place. The only implementation of the
    fold, for CPU and GPU tensors."""
    w = w_prep.double() if w_prep.dtype == torch.float64 else w_prep.float()
    k0, k1, k2 = w[:, 0], w[:, 1], w[:, 2]  # [Cout,3(kx),Cin]
    rows = torch.stack(  # [2(a),Cout,2(r),3(kx),Cin]
        [torch.stack([k0, k1 + k2], 1), torch.stack([k0 + k1, k2], 1)]
    )
    c0, c1, c2 = rows[..., 0, :], rows[..., 1, :], rows[..., 2, :]
    fold = torch.stack(  # [2(a),2(b),Cout,2(r),2(s),Cin]
        [torch.stack([c0, c1 + c2], -2), torch.stack([c0 + c1, c2], -2)], 1
    )
    fold = fold.reshape(4, *fold.shape[2:]).to(w_prep.dtype)
    if out is not None:
        out.copy_(fold)
        return out
    return fold.contiguous()


def ups2x_conv3x3(
    x: torch.Tensor,
    w_prep: torch.Tensor,
    bias: Optional[torch.Tensor],
    collect_gn: bool = False,
    wrap: Tuple[bool, bool] = (False, False),
    w_fold: Optional[torch.Tensor] = None,
    fold: bool = True,
) -> torch.Tensor:
    """Nearest-2x upsample fused into a 3x3 conv (VAE decoder / UNet
    Upsample): no 4x intermediate tensor. wrap = (height, width) wraps the
    conv's padding around the upsampled image. fold (the default) runs it
    as four 2x2 sub-pixel convs on the source image with the folded weights
    w_fold (fold_ups2x_weight(w_prep); computed here when absent - callers
    on a hot path cache it): 2.25x fewer FLOPs. fold=False keeps the 9-tap
    kernel. GPU-only entry."""
    if fold and w_fold is None:
        w_fold = fold_ups2x_weight(w_prep)
    y, gnp = ext().ups2x_conv3x3(
        x, w_prep, bias, collect_gn, bool(wrap[0]), bool(wrap[1]),
        w_fold if fold else None, bool(fold),
    )
    _attach_gn_partials(y, gnp)
    return y


# ---------------------------------------------------------------------------
# timestep embedding (sinusoidal)
# ---------------------------------------------------------------------------
def timestep_embedding(
    t: torch.Tensor, dim: int, max_period: float = 10000.0
) -> torch.Tensor:
    """[B] -> [B, dim] sin/cos embedding, fp32 (tiny; host-precomputable)."""
    half = dim // 2
    freqs = torch.exp(
        -math.log(max_period)
        * torch.arange(half, dtype=torch.float32, device=t.device)
        / half
    )
    args = t.float()[:, None] * freqs[None, :]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = F.pad(emb, (0, 1))
    return emb
