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
    the unmerge folded into the add, so the unmerged tensor never exists.

    Without gather, a width that is a multiple of 4 but not of 8 (embed 180,
    60), at most 256, runs the un-gated hab_tail_bf16_kernel."""
    d = x.shape[-1]
    if x.is_cuda and x.dtype == torch.bfloat16 and d % 8 == 0 and d <= 1536:
        if gather is not None:
            out = ext().add_layer_norm_gather(
                x, res, weight, bias, eps, gather.contiguous()
            )
        else:
            out = ext().add_layer_norm(x, res, weight, bias, eps)
        return out[0], out[1]
    if gather is None and x.is_cuda and x.dtype == torch.bfloat16 \
            and res.dtype == x.dtype and res.shape == x.shape \
            and d % 4 == 0 and d <= HAB_TAIL_MAX_C:
        return gated_add_layer_norm(x.contiguous(), res.contiguous(), None,
                                    None, weight, bias, eps)
    if gather is not None:
        res = _tome_gather_rows(res, gather)
    s = (x.float() + res.float()).to(x.dtype)
    return s, layer_norm(s, weight, bias, eps)


# ---------------------------------------------------------------------------
# token merging (ToMe) for the level-0 self-attention: 2x2 partition, cosine
# match, plan, merge, unmerge. Kernels in ops/hip/tome.hip and
# ops/hip/tome_plan.hip; every op has a
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


def tome_plan_supported(node_max, node_idx, h: int, w: int) -> bool:
    """True when tome_plan runs tome_plan_kernel on these inputs: contiguous
    fp32 / int32 GPU tensors [B, Ns] of a grid of at most 16384 tokens
    (128 x 128), which the kernel keeps in LDS as one row."""
    return bool(
        node_max.is_cuda and node_idx.is_cuda
        and node_max.dtype == torch.float32 and node_idx.dtype == torch.int32
        and node_max.dim() == 2 and node_idx.dim() == 2
        and node_max.is_contiguous() and node_idx.is_contiguous()
        and int(h) * int(w) <= ext().tome_plan_max_tokens()
    )


def tome_plan(node_max, node_idx, h: int, w: int, r: int,
              native: bool = True) -> TomePlan:
    """Select the r src tokens with the largest node_max (ties to the lower
    src position) and lay out the merge.

    GPU, tome_plan_supported(...): one launch of tome_plan_kernel. Larger
    grids, the CPU, and native=False (the oracle of the kernel and the
    composed route for comparisons): torch integer ops with static shapes on
    node_max's device, two stable sorts, a cumsum, a searchsorted and
    scatters to unique (or discarded) targets. The two routes return equal
    tensors. No host sync, no global atomics, so both capture into a
    hipGraph."""
    src, dst, inv = _tome_partition_all(h, w, node_max.device)
    ns, nd = src.numel(), dst.numel()
    bsz = node_max.shape[0]
    r = int(r)
    if tuple(node_max.shape) != (bsz, ns) or tuple(node_idx.shape) != (bsz, ns):
        raise ValueError(f"tome_plan: node_max/node_idx must be [B, {ns}]")
    if not 0 <= r <= ns:
        raise ValueError(f"tome_plan: r must lie in [0, {ns}] (got {r})")
    if native and tome_plan_supported(node_max, node_idx, h, w):
        slot, unm_tok, seg_start, members = ext().tome_plan(
            node_max, node_idx, src, dst, r
        )
        return TomePlan(int(h), int(w), r, slot, unm_tok, seg_start, members,
                        dst)
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
# wide head dims (256, 512): the VAE mid-block's flash kernel
# ---------------------------------------------------------------------------
_WIDE_DIMS = (256, 512)  # mirrors ext().attention_wide_supported


def _rows16(t: torch.Tensor) -> bool:
    """Unit stride in D and every row start 16-byte aligned."""
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0
            and all(t.shape[i] == 1 or t.stride(i) % 8 == 0 for i in range(3)))


def attention_wide_supported(q, k, v) -> bool:
    """True when attention_wide runs its kernel on these [B,H,S,D] views: on
    the GPU, bf16, head dim 256 or 512, unit stride in D and 16-byte-aligned
    rows. The predicate callers route by."""
    return bool(
        q.dim() == k.dim() == v.dim() == 4
        and q.is_cuda and k.is_cuda and v.is_cuda
        and q.dtype == k.dtype == v.dtype == torch.bfloat16
        and q.shape[-1] in _WIDE_DIMS
        and k.shape == v.shape and k.shape[-1] == q.shape[-1]
        and q.shape[:2] == k.shape[:2]
        and q.shape[2] >= 1 and k.shape[2] >= 1
        and _rows16(q) and _rows16(k) and _rows16(v)
    )


def attention_wide(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    scale: Optional[float] = None,
) -> torch.Tensor:
    """q [B,H,Sq,D], k/v [B,H,Sk,D] with D = 256 or 512 -> [B,H,Sq,D].

    GPU: flash_wide_bf16_kernel (ops/hip/attention_wide.hip): no score
    matrix in memory, v2's arithmetic (fp32 score scaling, one bf16 rounding
    of P and of the output). Strided views ([B,S,H,D] permuted, slices of a
    larger buffer) run with no copies. Anything the kernel does not take
    raises ValueError naming the argument; nothing is composed silently.
    CPU: the fp32 reference of attention().
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if not q.is_cuda:
        return attention(q, k, v, scale)
    name = "attention_wide"
    for nm, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 4:
            raise ValueError(f"{name}: {nm} must be [B,H,S,D], got "
                             f"{tuple(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"{name}: {nm} must be on the GPU like q")
        if t.dtype != torch.bfloat16:
            raise ValueError(f"{name}: {nm} must be bf16, got {t.dtype}")
    if q.shape[-1] not in _WIDE_DIMS:
        raise ValueError(f"{name}: q head dim {q.shape[-1]} has no wide "
                         f"kernel (expected one of {_WIDE_DIMS})")
    if k.shape != v.shape:
        raise ValueError(f"{name}: k {tuple(k.shape)} and v {tuple(v.shape)} "
                         "shapes differ")
    if k.shape[-1] != q.shape[-1] or k.shape[:2] != q.shape[:2]:
        raise ValueError(f"{name}: k {tuple(k.shape)} does not match q "
                         f"{tuple(q.shape)} in batch, heads or head dim")
    if q.shape[2] < 1 or k.shape[2] < 1:
        raise ValueError(f"{name}: q and k need at least one row")
    for nm, t in (("q", q), ("k", k), ("v", v)):
        if not _rows16(t):
            raise ValueError(f"{name}: {nm} needs unit stride in D and "
                             "16-byte-aligned rows")
    return ext().attention_wide(q, k, v, scale)


# ---------------------------------------------------------------------------
# shifted-window attention with a relative-position bias (SwinIR)
# ---------------------------------------------------------------------------
SWIN_WINDOW = 8
SWIN_DPAD = 32  # the kernel's head row: 30 channels padded by the model


def _swin_kernel_reason(qkv: torch.Tensor, bias: torch.Tensor) -> Optional[str]:
    """Why swin_attn_bf16_kernel does not take these (shape-checked)
    arguments, or None when it does."""
    if not (qkv.is_cuda and bias.is_cuda and qkv.device == bias.device):
        return "qkv and bias must be on the same GPU"
    if qkv.dtype != torch.bfloat16:
        return f"qkv must be bf16, got {qkv.dtype}"
    if bias.dtype != torch.float32:
        return f"bias must be fp32, got {bias.dtype}"
    if not bias.is_contiguous() or bias.data_ptr() % 16:
        return "bias must be contiguous and 16-byte aligned"
    if qkv.shape[5] != SWIN_DPAD:
        return (f"head dim {qkv.shape[5]} must be padded to Dp = "
                f"{SWIN_DPAD} (zero channels) by the caller")
    if qkv.stride(5) != 1 or qkv.data_ptr() % 16 or any(
            qkv.shape[i] != 1 and (qkv.stride(i) % 8 or qkv.stride(i) < 0)
            for i in range(5)):
        return ("qkv needs unit innermost stride and 16-byte-aligned head "
                "rows (outer strides multiples of 8)")
    return None


def _swin_check(qkv: torch.Tensor, bias: torch.Tensor, shift: int) -> None:
    name = "attention_swin"
    if qkv.dim() != 6 or qkv.shape[3] != 3:
        raise ValueError(f"{name}: qkv must be [B, H, W, 3, heads, Dp], got "
                         f"{tuple(qkv.shape)}")
    b, h, w, _, heads, _ = qkv.shape
    if b < 1 or heads < 1 or h < 1 or w < 1 or h % SWIN_WINDOW or w % SWIN_WINDOW:
        raise ValueError(f"{name}: the token grid {h} x {w} must be a "
                         f"multiple of the window ({SWIN_WINDOW})")
    n = SWIN_WINDOW * SWIN_WINDOW
    if tuple(bias.shape) != (heads, n, n):
        raise ValueError(f"{name}: bias must be [heads, {n}, {n}] = "
                         f"[{heads}, {n}, {n}] (window {SWIN_WINDOW}), got "
                         f"{tuple(bias.shape)}")
    if shift not in (0, SWIN_WINDOW // 2):
        raise ValueError(f"{name}: shift must be 0 or {SWIN_WINDOW // 2}, "
                         f"got {shift}")
    if not (qkv.is_floating_point() and bias.is_floating_point()):
        raise ValueError(f"{name}: qkv and bias must be floating point")


def attention_swin_supported(qkv: torch.Tensor, bias: torch.Tensor) -> bool:
    """True when attention_swin runs swin_attn_bf16_kernel on these
    arguments: qkv a bf16 [B, H, W, 3, heads, 32] GPU view with unit
    innermost stride and 16-byte-aligned head rows, H and W multiples of 8,
    bias a contiguous, 16-byte-aligned fp32 [heads, 64, 64] on the same
    GPU."""
    try:
        _swin_check(qkv, bias, 0)
    except ValueError:
        return False
    return _swin_kernel_reason(qkv, bias) is None


def _swin_region_mask(h: int, w: int, shift: int, device,
                      ws: int = SWIN_WINDOW) -> torch.Tensor:
    """[windows, ws*ws, ws*ws]: -100 where query and key lie in different
    regions of the shifted frame, built from the three row and three column
    slices."""
    img = torch.zeros(h, w, device=device)
    cnt = 0
    for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[hs, wsl] = cnt
            cnt += 1
    win = img.view(h // ws, ws, w // ws, ws).permute(0, 2, 1, 3)
    win = win.reshape(-1, ws * ws)
    diff = win[:, None, :] - win[:, :, None]
    return torch.zeros_like(diff).masked_fill(diff != 0, -100.0)


def _attention_swin_torch(qkv, bias, scale: float, shift: int) -> torch.Tensor:
    """The literal definition: roll, partition, bias and slice-built mask,
    softmax, reverse, roll back. Any head dim, any float dtype (bf16 and
    fp16 compute in fp32)."""
    ws = SWIN_WINDOW
    b, h, w, _, heads, d = qkv.shape
    cdt = qkv.dtype if qkv.dtype in (torch.float32, torch.float64) \
        else torch.float32
    x = qkv.to(cdt)
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    # partition: [B * windows, 64, 3, heads, d] -> q, k, v [B*win, heads, 64, d]
    x = x.reshape(b, h // ws, ws, w // ws, ws, 3, heads, d)
    x = x.permute(0, 1, 3, 2, 4, 5, 6, 7).reshape(-1, ws * ws, 3, heads, d)
    q, k, v = x.permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q * scale) @ k.transpose(-2, -1) + bias.to(cdt)[None]
    if shift:
        mask = _swin_region_mask(h, w, shift, qkv.device).to(cdt)
        nw = mask.shape[0]
        attn = attn.view(b, nw, heads, ws * ws, ws * ws) + mask[None, :, None]
        attn = attn.view(-1, heads, ws * ws, ws * ws)
    out = torch.softmax(attn, dim=-1) @ v           # [B*win, heads, 64, d]
    out = out.transpose(1, 2).reshape(b, h // ws, w // ws, ws, ws, heads * d)
    out = out.permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, heads * d)
    if shift:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out.to(qkv.dtype)


def attention_swin(
    qkv: torch.Tensor,
    bias: torch.Tensor,
    scale: float,
    shift: int = 0,
    native: bool = True,
) -> torch.Tensor:
    """SwinIR's (shifted-)window attention over an un-partitioned token grid.

    qkv [B, H, W, 3, heads, Dp] is the QKV projection of the grid (a view of
    the GEMM output is fine), bias [heads, 64, 64] the gathered relative
    position bias; windows are 8 x 8, shift is 0 or 4. Returns
    [B, H, W, heads * Dp] with every query's row at its un-shifted token, so
    the caller rolls, partitions and reverses nothing.

    bf16 qkv on the GPU runs swin_attn_bf16_kernel
    (ops/hip/attention_swin.hip) and must satisfy its contract (Dp = 32,
    contiguous fp32 bias, aligned head rows): what it does not take raises
    ValueError with the reason, nothing is composed silently. CPU tensors,
    other dtypes and native=False take the literal torch definition, which
    the model's reference route uses.
    """
    shift = int(shift)
    _swin_check(qkv, bias, shift)
    if native and qkv.is_cuda and qkv.dtype == torch.bfloat16:
        why = _swin_kernel_reason(qkv, bias)
        if why is not None:
            raise ValueError(f"attention_swin: {why}")
        return ext().attention_swin(qkv, bias, float(scale), shift)
    return _attention_swin_torch(qkv, bias, float(scale), shift)


# ---------------------------------------------------------------------------
# HAT: window-16 self-attention and overlapping cross-attention (kw 24)
# ---------------------------------------------------------------------------
HAT_WINDOW = 16
_HAT_KW = (HAT_WINDOW, HAT_WINDOW * 3 // 2)


def _hat_offset_gather(kw: int, device) -> torch.Tensor:
    """[256, kw*kw] positions of (query, key) pairs in a flattened
    [kw+15, kw+15] offset table: (ky - qy + 15) * R + kx - qx + 15."""
    r = kw + HAT_WINDOW - 1
    q = torch.arange(HAT_WINDOW, device=device)
    k = torch.arange(kw, device=device)
    d = k[None, :] - q[:, None] + HAT_WINDOW - 1             # [16, kw]
    pos = d[:, None, :, None] * r + d[None, :, None, :]      # [qy, qx, ky, kx]
    return pos.reshape(HAT_WINDOW * HAT_WINDOW, kw * kw)


def window_bias_offsets(table: torch.Tensor, index: torch.Tensor,
                        kw: int) -> torch.Tensor:
    """A HAT relative-position bias as the offset table the kernel takes:
    [heads, kw+15, kw+15], entry [ky - qy + 15, kx - qx + 15] the bias of key
    (ky, kx) of the kw x kw key patch for query (qy, qx) of the 16 x 16 window.

    table is [T, heads], index [256, kw*kw] as the model stores them (negative
    entries address the table from its end). Each offset is read from one
    (query, key) pair that has it; the expansion is then checked against
    table[index] for every pair, and an index that is not translation
    invariant raises ValueError naming the first mismatch."""
    n = HAT_WINDOW * HAT_WINDOW
    if kw not in _HAT_KW:
        raise ValueError(f"window_bias_offsets: kw must be one of {_HAT_KW}")
    if table.dim() != 2 or tuple(index.shape) != (n, kw * kw):
        raise ValueError(
            f"window_bias_offsets: table must be [T, heads] and index "
            f"[{n}, {kw * kw}], got {tuple(table.shape)} and "
            f"{tuple(index.shape)}")
    index = index.to(table.device).long()
    if index.min() < -table.shape[0] or index.max() >= table.shape[0]:
        raise ValueError("window_bias_offsets: index entries outside the "
                         f"table's {table.shape[0]} rows")
    r = kw + HAT_WINDOW - 1
    pos = _hat_offset_gather(kw, table.device)
    slot = torch.empty(r * r, dtype=torch.long, device=table.device)
    slot[pos.reshape(-1)] = index.reshape(-1)     # one pair per offset wins
    bad = (slot[pos] != index).nonzero()
    if bad.numel():
        q, k = (int(v) for v in bad[0])
        raise ValueError(
            f"window_bias_offsets: the index is not translation invariant: "
            f"query {q}, key {k} has entry {int(index[q, k])} but another "
            f"pair at the same offset has {int(slot[pos[q, k]])}")
    return table[slot].view(r, r, -1).permute(2, 0, 1).contiguous()


def _hat_kernel_reason(qkv: torch.Tensor, bias_off: torch.Tensor
                       ) -> Optional[str]:
    """Why hat_attn_bf16_kernel does not take these (shape-checked)
    arguments, or None when it does."""
    if not (qkv.is_cuda and bias_off.is_cuda
            and qkv.device == bias_off.device):
        return "qkv and bias_off must be on the same GPU"
    if qkv.dtype != torch.bfloat16:
        return f"qkv must be bf16, got {qkv.dtype}"
    if bias_off.dtype != torch.float32:
        return f"bias_off must be fp32, got {bias_off.dtype}"
    if not bias_off.is_contiguous():
        return "bias_off must be contiguous"
    if qkv.shape[5] != SWIN_DPAD:
        return (f"head dim {qkv.shape[5]} must be padded to Dp = "
                f"{SWIN_DPAD} (zero channels) by the caller")
    if qkv.stride(5) != 1 or qkv.data_ptr() % 16 or any(
            qkv.shape[i] != 1 and (qkv.stride(i) % 8 or qkv.stride(i) < 0)
            for i in range(5)):
        return ("qkv needs unit innermost stride and 16-byte-aligned head "
                "rows (outer strides multiples of 8)")
    return None


def _hat_check(qkv, bias_off, shift: int, kw: int) -> None:
    name = "attention_hat"
    if kw not in _HAT_KW:
        raise ValueError(f"{name}: kw must be one of {_HAT_KW}, got {kw}")
    if qkv.dim() != 6 or qkv.shape[3] != 3:
        raise ValueError(f"{name}: qkv must be [B, H, W, 3, heads, Dp], got "
                         f"{tuple(qkv.shape)}")
    b, h, w, _, heads, _ = qkv.shape
    if b < 1 or heads < 1 or h < 1 or w < 1 or h % HAT_WINDOW or w % HAT_WINDOW:
        raise ValueError(f"{name}: the token grid {h} x {w} must be a "
                         f"multiple of the window ({HAT_WINDOW})")
    r = kw + HAT_WINDOW - 1
    if tuple(bias_off.shape) != (heads, r, r):
        raise ValueError(f"{name}: bias_off must be [{heads}, {r}, {r}] at kw "
                         f"{kw} (window_bias_offsets), got "
                         f"{tuple(bias_off.shape)}")
    if shift not in (0, HAT_WINDOW // 2) or (shift and kw != HAT_WINDOW):
        raise ValueError(f"{name}: shift must be 0, or {HAT_WINDOW // 2} at "
                         f"kw {HAT_WINDOW}; got shift {shift}, kw {kw}")
    if not (qkv.is_floating_point() and bias_off.is_floating_point()):
        raise ValueError(f"{name}: qkv and bias_off must be floating point")


def attention_hat_supported(qkv: torch.Tensor, bias_off: torch.Tensor,
                            kw: int = HAT_WINDOW) -> bool:
    """True when attention_hat runs hat_attn_bf16_kernel on these arguments:
    qkv a bf16 [B, H, W, 3, heads, 32] GPU view with unit innermost stride
    and 16-byte-aligned head rows, H and W multiples of 16, bias_off a
    contiguous fp32 [heads, kw+15, kw+15] on the same GPU, kw 16 or 24."""
    try:
        _hat_check(qkv, bias_off, 0, kw)
    except ValueError:
        return False
    return _hat_kernel_reason(qkv, bias_off) is None


def _attention_hat_torch(qkv, bias_off, scale: float, shift: int,
                         kw: int) -> torch.Tensor:
    """The literal definition. kw 16: roll, partition, bias and slice-built
    mask, softmax, reverse, roll back. kw 24: partitioned queries against
    F.unfold(kernel 24, stride 16, padding 4) of K and V. The bias is
    bias_off expanded with one gather. Any head dim, any float dtype (bf16
    and fp16 compute in fp32)."""
    ws = HAT_WINDOW
    b, h, w, _, heads, d = qkv.shape
    nq, nwin = ws * ws, (h // ws) * (w // ws)
    cdt = qkv.dtype if qkv.dtype in (torch.float32, torch.float64) \
        else torch.float32
    x = qkv.to(cdt)
    bias = bias_off.to(cdt).flatten(1)[:, _hat_offset_gather(kw, qkv.device)]
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))

    def windows(t):     # [B, H, W, heads, d] -> [B, windows, heads, 256, d]
        t = t.reshape(b, h // ws, ws, w // ws, ws, heads, d)
        return t.permute(0, 1, 3, 5, 2, 4, 6).reshape(b, nwin, heads, nq, d)

    def patches(t):     # the same, 24 x 24 patches with zeros outside
        t = t.permute(0, 3, 4, 1, 2).reshape(b, heads * d, h, w)
        t = F.unfold(t, kernel_size=kw, stride=ws, padding=(kw - ws) // 2)
        return t.view(b, heads, d, kw * kw, nwin).permute(0, 4, 1, 3, 2)

    q = windows(x[:, :, :, 0])
    if kw == ws:
        k, v = windows(x[:, :, :, 1]), windows(x[:, :, :, 2])
    else:
        k, v = patches(x[:, :, :, 1]), patches(x[:, :, :, 2])
    attn = (q * scale) @ k.transpose(-2, -1) + bias[None, None]
    if shift:
        mask = _swin_region_mask(h, w, shift, qkv.device, ws).to(cdt)
        attn = attn + mask[None, :, None]
    out = torch.softmax(attn, dim=-1) @ v       # [B, windows, heads, 256, d]
    out = out.view(b, h // ws, w // ws, heads, ws, ws, d)
    out = out.permute(0, 1, 4, 2, 5, 3, 6).reshape(b, h, w, heads * d)
    if shift:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out.to(qkv.dtype)


def attention_hat(
    qkv: torch.Tensor,
    bias_off: torch.Tensor,
    scale: float,
    shift: int = 0,
    kw: int = HAT_WINDOW,
    native: bool = True,
) -> torch.Tensor:
    """HAT's attention over an un-partitioned token grid: 16 x 16 query
    windows against their own window (kw 16, shift 0 or 8 with Swin's region
    mask) or against the 24 x 24 patch centred on the window (kw 24, the
    overlapping cross-attention; positions outside the grid are present keys
    with k = v = 0).

    qkv [B, H, W, 3, heads, Dp] is the QKV projection of the grid (a view of
    the GEMM output is fine), bias_off [heads, kw+15, kw+15] the relative
    position bias by offset (window_bias_offsets). Returns
    [B, H, W, heads * Dp] with every query's row at its own token.

    bf16 qkv on the GPU runs hat_attn_bf16_kernel (ops/hip/attention_hat.hip)
    and must satisfy its contract (Dp = 32, contiguous fp32 bias_off, aligned
    head rows): what it does not take raises ValueError with the reason,
    nothing is composed silently. CPU tensors, other dtypes and native=False
    take the literal torch definition, which the model's reference route uses.
    """
    shift, kw = int(shift), int(kw)
    _hat_check(qkv, bias_off, shift, kw)
    if native and qkv.is_cuda and qkv.dtype == torch.bfloat16:
        why = _hat_kernel_reason(qkv, bias_off)
        if why is not None:
            raise ValueError(f"attention_hat: {why}")
        return ext().attention_hat(qkv, bias_off, float(scale), shift, kw)
    return _attention_hat_torch(qkv, bias_off, float(scale), shift, kw)


# ---------------------------------------------------------------------------
# the MLP half of a Swin block: fc1 + GELU + fc2 + residual (+ LayerNorm)
# ---------------------------------------------------------------------------
SWIN_MLP_CHUNK = 32   # hidden units the kernel walks at a time
SWIN_MLP_MAX_C = 256


def _swin_mlp_cpad(c: int) -> int:
    """The kernel instantiation's column count for embed width c."""
    return 192 if c <= 192 else 256


def swin_mlp_width_supported(c: int) -> bool:
    """True when swin_mlp_bf16_kernel has an instantiation for embed width c:
    a multiple of 4 (8-byte-aligned rows), at most 256."""
    return c % 4 == 0 and 4 <= c <= SWIN_MLP_MAX_C


def swin_mlp_prepare(w1, b1, w2, b2):
    """Pad an MLP's weights once for swin_mlp_bf16_kernel.

    w1 [hidden, C], b1 [hidden], w2 [C, hidden], b2 [C] (nn.Linear layout) ->
      w1p [Hp, CPAD]        w1p[j, c] = w1[j, c], zero elsewhere
      b1p [Hp] fp32
      w2p [Hp/32, CPAD, 32] w2p[j, c, k] = w2[c, 32 j + k], zero elsewhere
                            (hidden chunk j as [column][hidden], the tile the
                            kernel stages)
      b2p [C] fp32
    with Hp the hidden size rounded up to 32 (360 -> 384) and CPAD 192 for
    C <= 192, else 256. The invariant: a padded hidden unit has zero w1 row
    and zero b1, so its activation is gelu(0) = 0, and it meets zero w2
    entries; padded columns have zero weights on both sides."""
    hidden, c = w1.shape
    if tuple(w2.shape) != (c, hidden) or tuple(b1.shape) != (hidden,) \
            or tuple(b2.shape) != (c,):
        raise ValueError(
            f"swin_mlp_prepare: w1 {tuple(w1.shape)}, b1 {tuple(b1.shape)}, "
            f"w2 {tuple(w2.shape)}, b2 {tuple(b2.shape)} are not fc1 "
            "[hidden, C] / fc2 [C, hidden] with their biases")
    if not swin_mlp_width_supported(c):
        raise ValueError(f"swin_mlp_prepare: C = {c} must be a multiple of 4, "
                         f"at most {SWIN_MLP_MAX_C}")
    cpad = _swin_mlp_cpad(c)
    hp = -(-hidden // SWIN_MLP_CHUNK) * SWIN_MLP_CHUNK
    w1p = F.pad(w1, (0, cpad - c, 0, hp - hidden)).contiguous()
    w2p = F.pad(w2, (0, hp - hidden, 0, cpad - c)).view(
        cpad, hp // SWIN_MLP_CHUNK, SWIN_MLP_CHUNK).permute(1, 0, 2).contiguous()
    b1p = F.pad(b1.float(), (0, hp - hidden)).contiguous()
    return w1p, b1p, w2p, b2.float().contiguous()


def _swin_mlp_kernel_reason(x, res, w1p, w2p) -> Optional[str]:
    """Why swin_mlp_bf16_kernel does not take these, or None when it does."""
    if not (x.is_cuda and all(t.is_cuda and t.device == x.device
                              for t in (res, w1p, w2p))):
        return "x, res and the weights must be on the same GPU"
    if any(t.dtype != torch.bfloat16 for t in (x, res, w1p, w2p)):
        return "x, res and the weights must be bf16"
    c = x.shape[-1]
    if not swin_mlp_width_supported(c):
        return (f"C = {c} must be a multiple of 4, at most {SWIN_MLP_MAX_C} "
                "(8-byte-aligned rows, one instantiation of 192 or 256 "
                "columns)")
    if res.shape != x.shape:
        return f"res {tuple(res.shape)} must have x's shape {tuple(x.shape)}"
    # rows are read in 8-byte pieces at every C; the 16-byte stores go to
    # outputs the extension allocates
    if not (x.is_contiguous() and res.is_contiguous()) \
            or x.data_ptr() % 8 or res.data_ptr() % 8:
        return "x and res must be contiguous and 8-byte aligned"
    cpad = _swin_mlp_cpad(c)
    if w1p.dim() != 2 or w1p.shape[1] != cpad \
            or w1p.shape[0] % SWIN_MLP_CHUNK or w1p.shape[0] < SWIN_MLP_CHUNK \
            or tuple(w2p.shape) != (w1p.shape[0] // SWIN_MLP_CHUNK, cpad,
                                    SWIN_MLP_CHUNK):
        return (f"weights must be padded by swin_mlp_prepare to w1p [Hp, "
                f"{cpad}] and w2p [Hp/32, {cpad}, 32], got "
                f"{tuple(w1p.shape)} and {tuple(w2p.shape)}")
    if not (w1p.is_contiguous() and w2p.is_contiguous()) \
            or w1p.data_ptr() % 16 or w2p.data_ptr() % 16:
        return "padded weights must be contiguous and 16-byte aligned"
    return None


def _swin_mlp_vector_reason(x, w1p, b1p, b2, ln_weight,
                            ln_bias) -> Optional[str]:
    """Why swin_mlp_bf16_kernel does not take one of its fp32 vectors (b1p
    [Hp], the rest [C]; the norm's pair may be None), or None when it does."""
    c = x.shape[-1]
    vectors = [("b1", b1p, w1p.shape[0]), ("b2", b2, c)]
    if ln_weight is not None:
        vectors += [("ln_weight", ln_weight, c), ("ln_bias", ln_bias, c)]
    for name, t, n in vectors:
        if not (t.is_cuda and t.device == x.device):
            return f"{name} must be on x's GPU"
        if t.dtype != torch.float32:
            return f"{name} must be fp32, got {t.dtype}"
        if tuple(t.shape) != (n,):
            return f"{name} must be [{n}], got {tuple(t.shape)}"
        if not t.is_contiguous() or t.data_ptr() % 16:
            return f"{name} must be contiguous and 16-byte aligned"
    return None


def swin_mlp_supported(x, res, w1p, w2p) -> bool:
    """True when swin_mlp runs swin_mlp_bf16_kernel on these: contiguous,
    8-byte-aligned bf16 x and res of one shape on the GPU, C % 4 == 0,
    C <= 256, weights as swin_mlp_prepare leaves them."""
    return _swin_mlp_kernel_reason(x, res, w1p, w2p) is None


def swin_mlp(x, res, w1, b1, w2, b2, ln_weight=None, ln_bias=None,
             eps: float = 1e-5, native: bool = True):
    """(s, LayerNorm(s)) with s = res + fc2(gelu(fc1(x))), the MLP half of a
    Swin block and the norm that follows it, over [..., C] token rows. The
    second result is None when no norm weights are given.

    bf16 x on the GPU with native=True runs swin_mlp_bf16_kernel
    (ops/hip/swin_mlp.hip) and takes the weights as swin_mlp_prepare leaves
    them (b1, b2 and the norm's tensors fp32): the hidden activation stays in
    registers, rounded to bf16 once, and the norm is taken from the fp32 sum.
    What the kernel does not take raises ValueError with the reason; nothing
    is composed silently. CPU tensors, other dtypes and native=False take the
    literal torch route on UNPADDED nn.Linear weights."""
    if (ln_weight is None) != (ln_bias is None):
        raise ValueError("swin_mlp: give both ln_weight and ln_bias or neither")
    if native and x.is_cuda and x.dtype == torch.bfloat16:
        why = _swin_mlp_kernel_reason(x, res, w1, w2) \
            or _swin_mlp_vector_reason(x, w1, b1, b2, ln_weight, ln_bias)
        if why is not None:
            raise ValueError(f"swin_mlp: {why}")
        c = x.shape[-1]
        out = ext().swin_mlp(x.view(-1, c), res.view(-1, c), w1, b1, w2, b2,
                             ln_weight, ln_bias, eps)
        return out[0].view(x.shape), \
            (out[1].view(x.shape) if len(out) > 1 else None)
    s = res + F.linear(F.gelu(F.linear(x, w1, b1)), w2, b2)
    if ln_weight is None:
        return s, None
    return s, F.layer_norm(s, (s.shape[-1],), ln_weight, ln_bias, eps)


# ---------------------------------------------------------------------------
# the window-attention half of a Swin-Conv block (SCUNet): LN1, QKV, biased
# and masked window attention, proj, residual and LN2 in one kernel
# ---------------------------------------------------------------------------
WINDOW_BLOCK_WIDTHS = (32, 64)  # mirrors ext().window_block_attn_supported_width
WINDOW_BLOCK_HEAD = 32


def window_attn_block_prepare(wqkv: torch.Tensor, wproj: torch.Tensor):
    """The QKV weight [3C, C] and the proj weight [C, C] (nn.Linear layout)
    as window_block_attn_bf16_kernel stages them: flat, one contiguous 1 KB
    block per MFMA fragment, block (tile, step) holding
    w[32 tile + lane % 32][16 step + 8 (lane // 32) + j] at [lane][j].
    Callers cache the pair per weight version."""
    if wproj.dim() != 2 or wproj.shape[0] != wproj.shape[1] \
            or tuple(wqkv.shape) != (3 * wproj.shape[0], wproj.shape[0]):
        raise ValueError(
            f"window_attn_block_prepare: wqkv {tuple(wqkv.shape)} and wproj "
            f"{tuple(wproj.shape)} are not [3C, C] and [C, C]")
    c = wproj.shape[0]
    if c not in WINDOW_BLOCK_WIDTHS:
        raise ValueError(f"window_attn_block_prepare: C = {c} must be one of "
                         f"{WINDOW_BLOCK_WIDTHS}")

    def frag(w):
        return w.detach().view(w.shape[0] // 32, 32, c // 16, 2, 8).permute(
            0, 2, 3, 1, 4).contiguous().view(-1)

    return frag(wqkv), frag(wproj)


def _wb_view_reason(name: str, t: torch.Tensor) -> Optional[str]:
    if t.stride(3) != 1 or t.data_ptr() % 16 or any(
            t.shape[i] != 1 and (t.stride(i) % 8 or t.stride(i) < 0)
            for i in range(3)):
        return (f"{name} needs unit channel stride, 16-byte-aligned rows and "
                "pixel strides that are multiples of 8")
    return None


def _wb_kernel_reason(x, y_out, n2_out) -> Optional[str]:
    """Why window_block_attn_bf16_kernel does not take these views, or None
    when it does."""
    if x.dim() != 4:
        return f"x must be [B, H, W, C], got {tuple(x.shape)}"
    if not (x.is_cuda and x.dtype == torch.bfloat16):
        return f"x must be bf16 on the GPU, got {x.dtype} on {x.device}"
    b, h, w, c = x.shape
    if c not in WINDOW_BLOCK_WIDTHS:
        return (f"C = {c} must be one of {WINDOW_BLOCK_WIDTHS} (the weights "
                "stay in LDS; wider branches run composed)")
    if b < 1 or h < 8 or w < 8 or h % 8 or w % 8:
        return f"the token grid {h} x {w} must be a multiple of the window (8)"
    for name, t in (("x", x), ("y_out", y_out), ("n2_out", n2_out)):
        if t.shape != x.shape or t.dtype != x.dtype or t.device != x.device:
            return f"{name} must be a bf16 {tuple(x.shape)} on x's GPU"
        why = _wb_view_reason(name, t)
        if why is not None:
            return why
    views = [t.permute(0, 3, 1, 2) for t in (x, y_out, n2_out)]
    if any(_dense_overlap(views[i], views[j]) != "disjoint"
           for i, j in ((1, 0), (2, 0), (1, 2))):
        return "x, y_out and n2_out must not share memory"
    return None


def window_attn_block_supported(x, y_out, n2_out) -> bool:
    """True when window_attn_block runs window_block_attn_bf16_kernel on
    these: bf16 [B, H, W, C] views on one GPU, C 32 or 64, H and W multiples
    of 8, unit channel stride, 16-byte-aligned rows, pixel strides that are
    multiples of 8 (channel slices of NHWC buffers qualify), no shared
    memory. The routing predicate."""
    return _wb_kernel_reason(x, y_out, n2_out) is None


def _window_attn_block_torch(x, ln1_w, ln1_b, wqkv, bqkv, rel, wproj, bproj,
                             ln2_w, ln2_b, scale, shift, eps):
    """The literal definition (SCUNet's WMSA between its two norms): roll,
    partition, rel gathered by `relation`, an -inf mask filled by slices,
    softmax, reverse, roll back."""
    p = SWIN_WINDOW
    b, h, w, c = x.shape
    heads = c // WINDOW_BLOCK_HEAD
    t = F.layer_norm(x, (c,), ln1_w, ln1_b, eps)
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    hw, ww = h // p, w // p
    t = t.view(b, hw, p, ww, p, c).permute(0, 1, 3, 2, 4, 5)
    t = t.reshape(b, hw * ww, p * p, c)
    qkv = F.linear(t, wqkv, bqkv).view(b, hw * ww, p * p, 3 * heads, -1)
    q, k, v = qkv.permute(3, 0, 1, 2, 4).chunk(3, dim=0)   # [heads, b, nw, 64, d]
    sim = torch.einsum("hbwpc,hbwqc->hbwpq", q, k) * scale
    coord = torch.tensor([[i, j] for i in range(p) for j in range(p)],
                         device=x.device)
    relation = coord[:, None, :] - coord[None, :, :] + p - 1
    sim = sim + rel.to(sim.dtype)[:, relation[:, :, 0],
                                  relation[:, :, 1]][:, None, None]
    if shift:
        mask = torch.zeros(hw, ww, p, p, p, p, dtype=torch.bool,
                           device=x.device)
        s = p - shift
        mask[-1, :, :s, :, s:, :] = True
        mask[-1, :, s:, :, :s, :] = True
        mask[:, -1, :, :s, :, s:] = True
        mask[:, -1, :, s:, :, :s] = True
        sim = sim.masked_fill(mask.view(1, 1, hw * ww, p * p, p * p),
                              float("-inf"))
    o = torch.einsum("hbwij,hbwjc->hbwic", torch.softmax(sim, dim=-1), v)
    o = o.permute(1, 2, 3, 0, 4).reshape(b, hw * ww, p * p, c)
    o = F.linear(o, wproj, bproj).view(b, hw, ww, p, p, c)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    y = x + o
    return y, F.layer_norm(y, (c,), ln2_w, ln2_b, eps)


def window_attn_block(x, ln1_w, ln1_b, wqkv, bqkv, rel, wproj, bproj, ln2_w,
                      ln2_b, scale: float, shift: int = 0, eps: float = 1e-5,
                      out=None, native: bool = True):
    """(y, LN2(y)) with y = x + proj(window_attention(LN1(x))): the attention
    half of a Swin-Conv block over a [B, H, W, C] token grid, windows 8 x 8,
    heads of 32 channels, shift 0 or 4, rel [heads, 15, 15] read by the
    offset of key from query. QKV output channels are (t * heads + h) * 32 + c.

    bf16 x on the GPU with native=True runs window_block_attn_bf16_kernel
    (ops/hip/window_block.hip) on wqkv and wproj as
    window_attn_block_prepare leaves them, with fp32 vectors and rel; out is
    an optional (y, n2) pair of views to write. What the kernel does not take
    raises ValueError with the reason; nothing is composed silently. CPU
    tensors, other dtypes and native=False take the literal torch definition
    on the unprepared nn.Linear weights."""
    name = "window_attn_block"
    shift = int(shift)
    if x.dim() != 4:
        raise ValueError(f"{name}: x must be [B, H, W, C], got "
                         f"{tuple(x.shape)}")
    b, h, w, c = x.shape
    if shift not in (0, SWIN_WINDOW // 2):
        raise ValueError(f"{name}: shift must be 0 or {SWIN_WINDOW // 2}, got "
                         f"{shift}")
    if c % WINDOW_BLOCK_HEAD or c < WINDOW_BLOCK_HEAD:
        raise ValueError(f"{name}: C = {c} must be a multiple of the head "
                         f"dim ({WINDOW_BLOCK_HEAD})")
    if h < 1 or w < 1 or h % SWIN_WINDOW or w % SWIN_WINDOW:
        raise ValueError(f"{name}: the token grid {h} x {w} must be a "
                         f"multiple of the window ({SWIN_WINDOW})")
    heads = c // WINDOW_BLOCK_HEAD
    if tuple(rel.shape) != (heads, 15, 15):
        raise ValueError(f"{name}: rel must be [heads, 15, 15] = "
                         f"[{heads}, 15, 15], got {tuple(rel.shape)}")
    if native and x.is_cuda and x.dtype == torch.bfloat16:
        if out is None:
            out = (torch.empty(x.shape, dtype=x.dtype, device=x.device),
                   torch.empty(x.shape, dtype=x.dtype, device=x.device))
        y, n2 = out
        why = _wb_kernel_reason(x, y, n2)
        if why is None and not (
                wqkv.dtype == wproj.dtype == torch.bfloat16
                and wqkv.dim() == wproj.dim() == 1
                and wqkv.numel() == 3 * c * c and wproj.numel() == c * c):
            why = ("wqkv and wproj must be the flat bf16 pair of "
                   "window_attn_block_prepare")
        if why is None:
            for nm, t, n in (("ln1_w", ln1_w, c), ("ln1_b", ln1_b, c),
                             ("bqkv", bqkv, 3 * c), ("bproj", bproj, c),
                             ("ln2_w", ln2_w, c), ("ln2_b", ln2_b, c),
                             ("rel", rel, heads * 225)):
                if t.dtype != torch.float32 or t.numel() != n \
                        or not t.is_contiguous() or t.device != x.device:
                    why = f"{nm} must be contiguous fp32 of {n} values on x's GPU"
                    break
        if why is not None:
            raise ValueError(f"{name}: {why}")
        ext().window_block_attn(x, y, n2, ln1_w, ln1_b, wqkv, bqkv, rel, wproj,
                                bproj, ln2_w, ln2_b, float(scale), shift,
                                float(eps))
        return y, n2
    y, n2 = _window_attn_block_torch(x, ln1_w, ln1_b, wqkv, bqkv, rel, wproj,
                                     bproj, ln2_w, ln2_b, float(scale), shift,
                                     float(eps))
    if out is not None:
        out[0].copy_(y)
        out[1].copy_(n2)
        return out
    return y, n2


# ---------------------------------------------------------------------------
# the elementwise tail of a HAT block: channel-attention gate, the three-way
# residual sum and the norm behind it (ops/hip/hab_tail.hip)
# ---------------------------------------------------------------------------
HAB_TAIL_MAX_C = 256     # one 8-byte piece a lane: C / 4 <= 64
CHANNEL_GATE_MAX_S = 32  # squeeze width channel_gate_kernel holds


def _hab_rows(t: torch.Tensor) -> bool:
    return bool(t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous()
                and t.data_ptr() % 8 == 0)


def hab_tail_supported(*rows: torch.Tensor) -> bool:
    """True when hab_tail_bf16_kernel (and, for c, channel_pool_bf16_kernel)
    takes these token tensors: contiguous, 8-byte-aligned bf16 [..., C] of
    one shape on one GPU, C a multiple of 4, at most 256."""
    x = rows[0]
    c = x.shape[-1]
    return bool(x.numel() and all(_hab_rows(t) and t.shape == x.shape
                    and t.device == x.device for t in rows)
                and c % 4 == 0 and 4 <= c <= HAB_TAIL_MAX_C and have_ext())


def _f32_gpu(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    """t as a contiguous, 16-byte-aligned fp32 tensor on like's device."""
    t = t.detach().to(device=like.device, dtype=torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _channel_gate_check(c, w1, b1, w2, b2) -> None:
    if c.dim() != 4:
        raise ValueError("channel_gate: c must be [B, H, W, C], got "
                         f"{tuple(c.shape)}")
    ch = c.shape[-1]
    if ch % 4 or ch < 4:
        raise ValueError(f"channel_gate: C = {ch} must be a multiple of 4")
    if w1.dim() != 2 or w1.shape[1] != ch or w1.shape[0] < 1:
        raise ValueError(f"channel_gate: w1 {tuple(w1.shape)} must be "
                         f"[S, {ch}]")
    s = w1.shape[0]
    for name, t, shape in (("b1", b1, (s,)), ("w2", w2, (ch, s)),
                           ("b2", b2, (ch,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"channel_gate: {name} {tuple(t.shape)} must be "
                             f"{list(shape)}")


def channel_gate(c, w1, b1, w2, b2, scale: float = 1.0) -> torch.Tensor:
    """The per-channel gate of a squeeze-and-excitation block over [B, H, W,
    C] tokens: scale * sigmoid(w2 relu(w1 mean_hw(c) + b1) + b2), fp32
    [B, C]. w1 [S, C], b1 [S], w2 [C, S], b2 [C].

    Contiguous bf16 c on the GPU with C <= 256 and S <= 32 runs
    channel_pool_bf16_kernel and channel_gate_kernel: fixed-order sums, the
    same bits on every call. Everything else evaluates the formula in torch
    in fp32 (the CPU route and the oracle). A malformed argument raises
    ValueError."""
    _channel_gate_check(c, w1, b1, w2, b2)
    b, ch = c.shape[0], c.shape[-1]
    if hab_tail_supported(c) and w1.shape[0] <= CHANNEL_GATE_MAX_S:
        return ext().channel_gate(c.view(b, -1, ch), _f32_gpu(w1, c),
                                  _f32_gpu(b1, c), _f32_gpu(w2, c),
                                  _f32_gpu(b2, c), float(scale))
    mean = c.float().mean((1, 2))
    hidden = F.relu(F.linear(mean, w1.float(), b1.float()))
    return scale * torch.sigmoid(F.linear(hidden, w2.float(), b2.float()))


def gated_add_layer_norm(x, a, c, gate, weight, bias, eps: float = 1e-5):
    """(s, LayerNorm(s)) with s = (x + a) + gate[b] * c over [B, H, W, C]
    tokens, gate fp32 [B, C] (ops.channel_gate); c and gate both None gives
    s = x + a, ops.add_layer_norm without the width limit of its kernel.

    Contiguous bf16 tensors on the GPU with C % 4 == 0 and C <= 256 run
    hab_tail_bf16_kernel: one pass, fp32 math, the norm taken from the
    unrounded s. Everything else runs the same formula in torch, the sum
    rounded to x's dtype before the norm as add_layer_norm's fallback does.
    A malformed argument raises ValueError."""
    if (c is None) != (gate is None):
        raise ValueError("gated_add_layer_norm: give both c and gate or "
                         "neither")
    ch = x.shape[-1]
    if ch % 4 or ch < 4:
        raise ValueError(f"gated_add_layer_norm: C = {ch} must be a multiple "
                         "of 4")
    for name, t in (("a", a), ("c", c)):
        if t is not None and t.shape != x.shape:
            raise ValueError(f"gated_add_layer_norm: {name} {tuple(t.shape)} "
                             f"must have x's shape {tuple(x.shape)}")
    if gate is not None and (x.dim() < 2
                             or tuple(gate.shape) != (x.shape[0], ch)):
        raise ValueError(f"gated_add_layer_norm: gate {tuple(gate.shape)} "
                         f"must be [{x.shape[0]}, {ch}]")
    for name, t in (("weight", weight), ("bias", bias)):
        if tuple(t.shape) != (ch,):
            raise ValueError(f"gated_add_layer_norm: {name} "
                             f"{tuple(t.shape)} must be [{ch}]")
    rows = (x, a) if c is None else (x, a, c)
    if hab_tail_supported(*rows):
        hw = x.numel() // (x.shape[0] * ch) if c is not None else 1
        out = ext().hab_tail(
            x.view(-1, ch), a.view(-1, ch),
            None if c is None else c.view(-1, ch),
            None if c is None else _f32_gpu(gate, x),
            _f32_gpu(weight, x), _f32_gpu(bias, x), eps, hw)
        return out[0].view(x.shape), out[1].view(x.shape)
    s = x.float() + a.float()
    if c is not None:
        s = s + gate.float().view(
            (x.shape[0],) + (1,) * (x.dim() - 2) + (ch,)) * c.float()
    s = s.to(x.dtype)
    return s, layer_norm(s, weight, bias, eps)


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
# dense-block 3x3 conv on channel slices (the RRDBNet trunk, models/esrgan.py)
# ---------------------------------------------------------------------------
def _dense_nhwc(t: torch.Tensor) -> bool:
    """A channel slice of an NHWC buffer the dense kernel can address: unit
    channel stride, rows of W pixels, pixel and image strides that are
    multiples of 8 elements, a 16-byte-aligned base, offsets below 2^31."""
    n, c, h, w = t.shape
    ld = t.stride(3)
    return bool(
        t.stride(1) == 1 and ld >= c and ld % 8 == 0
        and t.stride(2) == w * ld and t.stride(0) % 8 == 0
        and (n == 1 or t.stride(0) >= h * w * ld)
        and t.data_ptr() % 16 == 0 and h * w * ld < 2 ** 31
    )


def _dense_overlap(out: torch.Tensor, t: torch.Tensor) -> str:
    """How out's channels relate to t's when both live in one storage:
    "disjoint", "identical", or "overlap" (anything else)."""
    if out.untyped_storage().data_ptr() != t.untyped_storage().data_ptr():
        return "disjoint"

    def extent(v):
        return ((v.shape[0] - 1) * v.stride(0) + (v.shape[2] - 1) * v.stride(2)
                + (v.shape[3] - 1) * v.stride(3) + v.shape[1])

    y0, t0 = out.storage_offset(), t.storage_offset()
    if y0 + extent(out) <= t0 or t0 + extent(t) <= y0:
        return "disjoint"
    ld = out.stride(3)
    if ld <= 0 or (t.stride(3), t.stride(2), t.stride(0)) != (
            ld, out.stride(2), out.stride(0)):
        return "overlap"
    cy, ct = y0 % ld, t0 % ld
    if (y0 - cy != t0 - ct or cy + out.shape[1] > ld
            or ct + t.shape[1] > ld):
        return "overlap"
    if cy + out.shape[1] <= ct or ct + t.shape[1] <= cy:
        return "disjoint"
    if cy == ct and out.shape[1] == t.shape[1]:
        return "identical"
    return "overlap"


def conv3x3_dense_supported(x, w_prep, out) -> bool:
    """True when conv3x3_dense runs conv3x3_dense_bf16_kernel on these views:
    bf16 on the GPU, Cin % 32 == 0 in [64, 256], Cout 32 or 64, N <= 65535,
    NHWC channel slices (unit channel stride, pixel strides % 8 == 0,
    16-byte-aligned bases), w_prep contiguous. The routing predicate."""
    return bool(
        x.is_cuda and out.is_cuda and w_prep.is_cuda
        and x.dtype == out.dtype == w_prep.dtype == torch.bfloat16
        and x.dim() == out.dim() == w_prep.dim() == 4
        and x.shape[1] % 32 == 0 and 64 <= x.shape[1] <= 256
        and out.shape[1] in (32, 64)
        and 1 <= x.shape[0] <= 65535 and x.shape[2] >= 1 and x.shape[3] >= 1
        and w_prep.is_contiguous() and w_prep.data_ptr() % 16 == 0
        and _dense_nhwc(x) and _dense_nhwc(out)
    )


def conv3x3_dense(
    x: torch.Tensor,
    w_prep: torch.Tensor,
    bias: Optional[torch.Tensor],
    out: torch.Tensor,
    *,
    alpha: float = 1.0,
    res1: Optional[torch.Tensor] = None,
    beta: float = 1.0,
    res2: Optional[torch.Tensor] = None,
    lrelu: Optional[float] = None,
) -> torch.Tensor:
    """out <- act(alpha * (conv3x3(x, w) + bias) + beta * res1 + res2), pad
    1, stride 1; act is LeakyReLU(lrelu) when lrelu is given. Written in
    place into `out`, which is returned.

    x, out, res1, res2 are [N, C, H, W] views with unit channel stride:
    channel slices of channels_last buffers (buf[:, :96], buf[:, 96:128]),
    possibly of ONE buffer, so a dense block runs with no concatenation. out
    must not share channels with x; a residual is disjoint from out or is
    exactly out's slice. w_prep is [Cout, 3, 3, Cin].

    GPU, conv3x3_dense_supported(x, w_prep, out): conv3x3_dense_bf16_kernel
    (ops/hip/conv_dense.hip), fp32 accumulate, one bf16 rounding. CPU, or
    when the predicate is false: the same formula with F.conv2d (fp32 math
    for bf16) copied into out. A bad argument raises ValueError naming it.
    """
    name = "conv3x3_dense"
    for nm, t in (("x", x), ("w_prep", w_prep), ("out", out)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: {nm} must be a 4-d tensor")
    n, cin, h, w = x.shape
    cout = out.shape[1]
    if min(n, cin, h, w) < 1:
        raise ValueError(f"{name}: x must be non-empty, got {tuple(x.shape)}")
    if tuple(w_prep.shape) != (cout, 3, 3, cin):
        raise ValueError(
            f"{name}: w_prep must be [Cout,3,3,Cin] = {(cout, 3, 3, cin)}, "
            f"got {tuple(w_prep.shape)}"
        )
    if bias is not None and bias.numel() != cout:
        raise ValueError(f"{name}: bias must hold {cout} values, got "
                         f"{bias.numel()}")
    views = [("out", out), ("res1", res1), ("res2", res2)]
    for nm, t in views:
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (n, cout, h, w):
            raise ValueError(
                f"{name}: {nm} must be {(n, cout, h, w)}, got "
                f"{tuple(t.shape) if torch.is_tensor(t) else type(t)}"
            )
    for nm, t in (("w_prep", w_prep), ("bias", bias)) + tuple(views):
        if t is None:
            continue
        if t.device != x.device:
            raise ValueError(f"{name}: {nm} is on {t.device}, x on {x.device}")
        if nm != "bias" and t.dtype != x.dtype:
            raise ValueError(f"{name}: {nm} is {t.dtype}, x is {x.dtype}")
    for nm, t in (("x", x),) + tuple(views):
        if t is not None and t.stride(1) != 1:
            raise ValueError(f"{name}: {nm} needs unit channel stride "
                             "(a channel slice of a channels_last buffer)")
    if _dense_overlap(out, x) != "disjoint":
        raise ValueError(f"{name}: out shares channels with x")
    for nm, t in views[1:]:
        if t is not None and _dense_overlap(out, t) == "overlap":
            raise ValueError(f"{name}: out partly overlaps {nm}; a residual "
                             "is disjoint from out or exactly its slice")
    if lrelu is not None and not isinstance(lrelu, (int, float)):
        raise ValueError(f"{name}: lrelu must be a slope or None")

    native = conv3x3_dense_supported(x, w_prep, out) and all(
        t is None or _dense_nhwc(t) for t in (res1, res2)
    )
    if native:
        return ext().conv3x3_dense(
            x, w_prep, bias, out, float(alpha), res1, float(beta), res2,
            lrelu is not None, float(lrelu or 0.0),
        )
    wide = x.dtype == torch.bfloat16
    up = (lambda t: t.float()) if wide else (lambda t: t)
    y = F.conv2d(
        up(x), up(w_prep).permute(0, 3, 1, 2),
        None if bias is None else bias.to(up(x).dtype), padding=1,
    )
    y = y * float(alpha)
    if res1 is not None:
        y = y + float(beta) * up(res1)
    if res2 is not None:
        y = y + up(res2)
    if lrelu is not None:
        y = F.leaky_relu(y, float(lrelu))
    out.copy_(y)
    return out


# ---------------------------------------------------------------------------
# 3x3 / 1x1 conv at channel widths that are no multiple of 64 (SwinIR's convs
# at embed 180 / 240 and their 60-wide stacks, models/swinir.py)
# ---------------------------------------------------------------------------
def _ragged_padded(cin: int, cout: int) -> Tuple[int, int]:
    """(ceil32(Cin), ceil64(Cout)): the prepared weight's padded widths."""
    return -(-cin // 32) * 32, -(-cout // 64) * 64


def conv_ragged_prepare(weight: torch.Tensor) -> torch.Tensor:
    """A conv weight [Cout, Cin, KS, KS] (KS 1 or 3) as conv_ragged reads it:
    [ceil64(Cout), KS, KS, ceil32(Cin)] in the weight's dtype, exact zeros
    outside the real block, so the kernel stages whole 16-byte pieces of
    whole 64-row tiles without masks. Callers cache it per weight version."""
    if (not torch.is_tensor(weight) or weight.dim() != 4
            or weight.shape[2] != weight.shape[3]
            or weight.shape[2] not in (1, 3)):
        raise ValueError("conv_ragged_prepare: weight must be "
                         "[Cout, Cin, KS, KS] with KS 1 or 3")
    cout, cin, ks, _ = weight.shape
    cinp, coutp = _ragged_padded(cin, cout)
    prep = weight.new_zeros(coutp, ks, ks, cinp)
    prep[:cout, :, :, :cin] = weight.detach().permute(0, 2, 3, 1)
    return prep


def _ragged_nhwc(t: torch.Tensor) -> bool:
    """A channel slice of an NHWC buffer the ragged kernel can address: unit
    channel stride, rows of W pixels, pixel and image strides that are
    multiples of 4 elements, an 8-byte-aligned base, offsets below 2^31."""
    n, c, h, w = t.shape
    ld = t.stride(3)
    return bool(
        t.stride(1) == 1 and ld >= c and ld % 4 == 0
        and t.stride(2) == w * ld
        and (n == 1 or (t.stride(0) % 4 == 0 and t.stride(0) >= h * w * ld))
        and t.data_ptr() % 8 == 0 and h * w * ld < 2 ** 31
    )


def conv_ragged_supported(x, weight, out) -> bool:
    """True when conv_ragged runs conv_ragged_bf16_kernel for the conv weight
    [Cout, Cin, KS, KS] on these views: bf16 on the GPU, KS 1 or 3, Cin and
    Cout multiples of 4 in [4, 512], N <= 65535, NHWC channel slices (unit
    channel stride, pixel strides % 4 == 0, 8-byte-aligned bases). The
    routing predicate."""
    return bool(
        x.is_cuda and out.is_cuda and weight.is_cuda
        and x.dtype == out.dtype == weight.dtype == torch.bfloat16
        and x.dim() == out.dim() == weight.dim() == 4
        and weight.shape[2] == weight.shape[3]
        and tuple(weight.shape[:2]) == (out.shape[1], x.shape[1])
        and ext().conv_ragged_supported_widths(
            x.shape[1], out.shape[1], weight.shape[2])
        and 1 <= x.shape[0] <= 65535 and x.shape[2] >= 1 and x.shape[3] >= 1
        and tuple(out.shape) == (x.shape[0], out.shape[1]) + tuple(x.shape[2:])
        and _ragged_nhwc(x) and _ragged_nhwc(out)
    )


def conv_ragged(
    x: torch.Tensor,
    w_prepared: torch.Tensor,
    bias: Optional[torch.Tensor],
    out: torch.Tensor,
    ksize: int = 3,
    lrelu: Optional[float] = None,
    res: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out <- act(conv(x, w) + bias) + res: a stride-1 "same" conv with a
    ksize x ksize kernel (3 or 1); act is LeakyReLU(lrelu) when lrelu is
    given. Written in place into `out`, which is returned.

    x, out, res are [N, C, H, W] views with unit channel stride (channel
    slices of channels_last buffers). out must not share channels with x;
    res is disjoint from out or exactly out's slice. w_prepared is
    conv_ragged_prepare(weight) for x's Cin and out's Cout.

    bf16 on the GPU with Cin and Cout multiples of 4 in [4, 512] and views
    the kernel can address: conv_ragged_bf16_kernel (ops/hip/conv_ragged.hip),
    fp32 accumulate, one bf16 rounding. CPU, or otherwise: the same formula
    with F.conv2d (fp32 math for bf16) on the unpadded block of w_prepared,
    copied into out. A bad argument raises ValueError naming it.
    """
    name = "conv_ragged"
    for nm, t in (("x", x), ("w_prepared", w_prepared), ("out", out)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: {nm} must be a 4-d tensor")
    if ksize not in (1, 3):
        raise ValueError(f"{name}: ksize must be 1 or 3, got {ksize!r}")
    n, cin, h, w = x.shape
    cout = out.shape[1]
    if min(n, cin, h, w) < 1:
        raise ValueError(f"{name}: x must be non-empty, got {tuple(x.shape)}")
    cinp, coutp = _ragged_padded(cin, cout)
    if tuple(w_prepared.shape) != (coutp, ksize, ksize, cinp):
        raise ValueError(
            f"{name}: w_prepared must be [ceil64(Cout),KS,KS,ceil32(Cin)] = "
            f"{(coutp, ksize, ksize, cinp)}, got {tuple(w_prepared.shape)}"
        )
    if bias is not None and bias.numel() != cout:
        raise ValueError(f"{name}: bias must hold {cout} values, got "
                         f"{bias.numel()}")
    views = [("out", out), ("res", res)]
    for nm, t in views:
        if t is None:
            continue
        if not torch.is_tensor(t) or tuple(t.shape) != (n, cout, h, w):
            raise ValueError(
                f"{name}: {nm} must be {(n, cout, h, w)}, got "
                f"{tuple(t.shape) if torch.is_tensor(t) else type(t)}"
            )
    for nm, t in (("w_prepared", w_prepared), ("bias", bias)) + tuple(views):
        if t is None:
            continue
        if t.device != x.device:
            raise ValueError(f"{name}: {nm} is on {t.device}, x on {x.device}")
        if nm != "bias" and t.dtype != x.dtype:
            raise ValueError(f"{name}: {nm} is {t.dtype}, x is {x.dtype}")
    for nm, t in (("x", x),) + tuple(views):
        if t is not None and t.stride(1) != 1:
            raise ValueError(f"{name}: {nm} needs unit channel stride "
                             "(a channel slice of a channels_last buffer)")
    if _dense_overlap(out, x) != "disjoint":
        raise ValueError(f"{name}: out shares channels with x")
    if res is not None and _dense_overlap(out, res) == "overlap":
        raise ValueError(f"{name}: out partly overlaps res; the residual is "
                         "disjoint from out or exactly its slice")
    if lrelu is not None and not isinstance(lrelu, (int, float)):
        raise ValueError(f"{name}: lrelu must be a slope or None")

    native = bool(
        x.is_cuda and x.dtype == torch.bfloat16
        and ext().conv_ragged_supported_widths(cin, cout, ksize)
        and n <= 65535 and w_prepared.is_contiguous()
        and w_prepared.data_ptr() % 16 == 0
        and all(t is None or _ragged_nhwc(t) for t in (x, out, res))
    )
    if native:
        return ext().conv_ragged(
            x, w_prepared, bias, out, int(ksize), res, lrelu is not None,
            float(lrelu or 0.0),
        )
    wide = x.dtype == torch.bfloat16
    up = (lambda t: t.float()) if wide else (lambda t: t)
    y = F.conv2d(
        up(x), up(w_prepared[:cout, :, :, :cin]).permute(0, 3, 1, 2),
        None if bias is None else bias.to(up(x).dtype), padding=ksize // 2,
    )
    if lrelu is not None:
        y = F.leaky_relu(y, float(lrelu))
    if res is not None:
        y = y + up(res)
    out.copy_(y)
    return out


# ---------------------------------------------------------------------------
# weight-stationary 3x3 conv at Cin 64 with a per-channel PReLU or a
# pixel-shuffle epilogue (the compact Real-ESRGAN upscalers, models/esrgan.py)
# ---------------------------------------------------------------------------
_CU_COUNT: dict = {}


def _cu_count(device) -> int:
    idx = torch.device(device).index
    idx = torch.cuda.current_device() if idx is None else idx
    if idx not in _CU_COUNT:
        _CU_COUNT[idx] = int(
            torch.cuda.get_device_properties(idx).multi_processor_count)
    return _CU_COUNT[idx]


def conv_compact_supported(x, w_prep) -> bool:
    """True when conv_compact runs conv_compact_bf16_kernel on these tensors:
    bf16 on the GPU, x [N, 64, H, W] channels_last with a 16-byte-aligned
    base and N * H * W * 64 < 2^31, w_prep a contiguous [64 or 48, 3, 3, 64].
    The routing predicate."""
    return bool(
        x.is_cuda and w_prep.is_cuda
        and x.dtype == w_prep.dtype == torch.bfloat16
        and x.dim() == w_prep.dim() == 4
        and x.shape[1] == 64 and min(x.shape) >= 1
        and tuple(w_prep.shape[1:]) == (3, 3, 64)
        and w_prep.shape[0] in (48, 64)
        and x.is_contiguous(memory_format=torch.channels_last)
        and w_prep.is_contiguous()
        and x.data_ptr() % 16 == 0 and w_prep.data_ptr() % 16 == 0
        and x.numel() < 2 ** 31
    )


def conv_compact(
    x: torch.Tensor,
    w_prep: torch.Tensor,
    bias: Optional[torch.Tensor],
    slope: Optional[torch.Tensor] = None,
    pre_slope: Optional[torch.Tensor] = None,
    shuffle_base: Optional[torch.Tensor] = None,
    blocks: Optional[int] = None,
) -> torch.Tensor:
    """A 3x3 / pad 1 / stride 1 conv of the compact (SRVGG) upscalers, with
    one of two epilogues; exactly one of `slope` and `shuffle_base` is given.

    slope [Cout]:  y = prelu(conv3x3(x', w) + bias, slope), [N, Cout, H, W]
    channels_last. With pre_slope [Cin], x' = prelu(x, pre_slope) rounded to
    x's dtype, as the separate activation pass it replaces would have stored
    it; otherwise x' = x.

    shuffle_base [N, 3, H, W] (any strides):  y = pixel_shuffle(conv3x3(x, w)
    + bias, 4) + nearest4x(shuffle_base), [N, 3, 4H, 4W] contiguous; Cout is
    48. The sum is formed before the one rounding.

    w_prep is [Cout, 3, 3, Cin]. GPU, conv_compact_supported(x, w_prep):
    conv_compact_bf16_kernel (ops/hip/conv_compact.hip), the layer's weights
    resident in LDS while a block walks output tiles, fp32 accumulate, one
    rounding; `blocks` caps the grid (default: the CU count). CPU, or when
    the predicate is false: the same formula with F.conv2d (fp32 math for
    bf16). A bad argument raises ValueError naming it.
    """
    name = "conv_compact"
    for nm, t in (("x", x), ("w_prep", w_prep)):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError(f"{name}: {nm} must be a 4-d tensor")
    n, cin, h, w = x.shape
    cout = w_prep.shape[0]
    if min(n, cin, h, w) < 1:
        raise ValueError(f"{name}: x must be non-empty, got {tuple(x.shape)}")
    if tuple(w_prep.shape) != (cout, 3, 3, cin):
        raise ValueError(
            f"{name}: w_prep must be [Cout,3,3,Cin] = {(cout, 3, 3, cin)}, "
            f"got {tuple(w_prep.shape)}"
        )
    if (slope is None) == (shuffle_base is None):
        raise ValueError(f"{name}: exactly one of slope and shuffle_base "
                         "must be given")
    if pre_slope is not None and slope is None:
        raise ValueError(f"{name}: pre_slope needs the slope epilogue")
    for nm, t, length in (("bias", bias, cout), ("slope", slope, cout),
                          ("pre_slope", pre_slope, cin)):
        if t is not None and (not torch.is_tensor(t) or t.dim() != 1
                              or t.numel() != length):
            raise ValueError(f"{name}: {nm} must be a vector of {length} "
                             "values")
    if shuffle_base is not None:
        if cout != 48:
            raise ValueError(f"{name}: the shuffle_base epilogue is "
                             f"PixelShuffle(4) of 48 channels, w_prep has "
                             f"{cout}")
        if (not torch.is_tensor(shuffle_base)
                or tuple(shuffle_base.shape) != (n, 3, h, w)):
            raise ValueError(f"{name}: shuffle_base must be {(n, 3, h, w)}")
    for nm, t in (("w_prep", w_prep), ("bias", bias), ("slope", slope),
                  ("pre_slope", pre_slope), ("shuffle_base", shuffle_base)):
        if t is None:
            continue
        if t.device != x.device:
            raise ValueError(f"{name}: {nm} is on {t.device}, x on {x.device}")
        if nm in ("w_prep", "shuffle_base") and t.dtype != x.dtype:
            raise ValueError(f"{name}: {nm} is {t.dtype}, x is {x.dtype}")
    if blocks is not None and (not isinstance(blocks, int) or blocks < 1):
        raise ValueError(f"{name}: blocks must be a positive int or None")

    if conv_compact_supported(x, w_prep) and cout == (
            48 if slope is None else 64):
        def vec(t):  # the kernel reads fp32 or bf16 as stored
            if t is None or (t.is_contiguous() and t.dtype in (
                    torch.float32, torch.bfloat16)):
                return t
            return t.float().contiguous()

        return ext().conv_compact(
            x, w_prep, vec(bias), vec(slope), vec(pre_slope), shuffle_base,
            int(blocks) if blocks is not None else _cu_count(x.device),
        )
    wide = x.dtype == torch.bfloat16
    up = (lambda t: t.float()) if wide else (lambda t: t)
    xin = up(x)
    if pre_slope is not None:
        xin = up(F.prelu(xin, pre_slope.to(xin.dtype)).to(x.dtype))
    y = F.conv2d(xin, up(w_prep).permute(0, 3, 1, 2),
                 None if bias is None else bias.to(xin.dtype), padding=1)
    if slope is not None:
        y = F.prelu(y, slope.to(y.dtype)).to(x.dtype)
        return y.contiguous(memory_format=torch.channels_last)
    y = F.pixel_shuffle(y, 4) + F.interpolate(
        up(shuffle_base), scale_factor=4, mode="nearest")
    return y.to(x.dtype).contiguous()


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
