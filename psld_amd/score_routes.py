"""Which kernel runs each 3x3 convolution, each pointwise GEMM and each batched product of the executor (score_exec.py /
score_tape.py): pure functions of integers and flags.  No tensors, no executor state, importable without a GPU.

Everything that depends on the kernel a 3x3 stride-1 pad-1 convolution runs on - the layout its producer writes (fp32 or
bf16 limb planes), the GroupNorm partial sums its epilogue can leave, the form of its data and weight gradients, whether a
block can read an unmaterialised concatenation - is decided HERE, once per residual block (``block_plan``), and consumed
by the executor.  The ``ops.conv3x3_*_supported`` / ``*_wanted`` / ``conv3x3_wgrad_*`` predicates are called from this
module only.

No cache of its own: ``ops.set_winograd`` / ``set_fused_gn`` / ``set_wgrad_winograd`` clear the predicates' caches and
nothing else, so a plan is rebuilt (a dozen cached lookups) for every block of every pass.
"""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional, Tuple

from . import ops

# routes of a 3x3 stride-1 pad-1 convolution (forward, data gradient, weight gradient)
WINO = "wino"           # Winograd F(2x2, 3x3): conv_wino.hip forward / data gradient, wgrad_wino.hip weight gradient
LIMB = "limb"           # direct bf16 limb kernels (conv_split.hip); the only route that reads ops.LimbPlanes
TILE = "tile"           # fp32 tile engine (ops.conv2d_nhwc / conv2d_wgrad_nhwc)
LIMB_TAIL = "limb_tail"  # pointwise and batched: the limb kernels with the last channel tile cut short (widths in steps of 32)
WINO_GN = "wino_gn"     # forward only: SiLU(GroupNorm(.)) applied inside the Winograd kernel's input staging
NONE = "none"           # weight gradient only: a two-source shape no kernel takes

# read-ahead padding at the end of a Winograd fragment buffer (the pad in psld_conv3x3_wino_frag_bytes): not part of the
# per-output-channel-tile fragments that _resblock_cat_bwd slices per source
WINO_FRAG_PAD_BYTES = 16384

_RESIDENT_BLOCKS = 512  # 256 CUs x 2 workgroups (64-72 KB LDS each) of the tile kernels


@functools.lru_cache(maxsize=None)
def _pick_nsplit(tiles: int, k: int, min_k: int = 256, resident: int = _RESIDENT_BLOCKS) -> int:
    """Split-K factor of a weight-gradient GEMM: fill whole rounds of resident workgroups (a 1.5-round
    grid wastes a quarter of the machine) while keeping >= ``min_k`` K per split."""
    max_split = max(1, k // min_k)
    best, best_eff = 1, 0.0
    for ns in range(1, min(max_split, 128) + 1):
        blocks = tiles * ns
        rounds = -(-blocks // resident)
        eff = blocks / (rounds * resident)
        if eff > best_eff + 0.02:
            best, best_eff = ns, eff
    return best


def _tn_split(m: int, n: int, k: int) -> int:
    """K ranges of a pointwise limb weight gradient (128x128 tiles, the last ones cut short on the tail route; two
    workgroups resident per CU)."""
    ktiles = k // 32
    nsplit = _pick_nsplit(-(-m // 128) * -(-n // 128), k, min_k=128, resident=512)
    per = -(-ktiles // nsplit)
    return -(-ktiles // per)                       # every slab non-empty


def wgrad_limb_nsplit(cout: int, cin: int, b: int, h: int, w: int, planes: bool) -> int:
    """K ranges of a direct limb 3x3 weight gradient (``planes``: its x operand is held as limb planes)."""
    ktiles = b * h * w // 32
    # resident workgroups: 64-channel tiles 3 per CU (46 KB LDS); 128-channel tiles 2 per CU with x as limb planes
    # (dwgrad_kernel<4, true>), ONE 512-thread workgroup per CU for fp32 x (the wave-specialised dwgrad_ws_kernel)
    co_tile = ops.conv3x3_wgrad_split_cout_tile(cout)
    resident = 768 if co_tile == 64 else (512 if planes else 256)
    nsplit = _pick_nsplit((cout // co_tile) * (cin // 64) * 3, ktiles * 32, min_k=128, resident=resident)
    per = -(-ktiles // nsplit)
    return -(-ktiles // per)                       # every slab non-empty


def wino_wanted(c1: int, c2: int, b: int, h: int, w: int, cout: int) -> bool:
    """ops.conv3x3_wino_wanted counting the launches that fill the chip only with their channel chunks split over workgroups
    (the 8x8 level at B=128, the 16x16 level at B=16).  The executor asks through its own ``wino_wanted`` method (which
    calls this) and hands that method to the functions below as ``wino``."""
    return ops.conv3x3_wino_wanted(c1, c2, b, h, w, cout, True)


def limb_takes(split: bool, c1: int, c2: int, b: int, h: int, w: int, cout: int) -> bool:
    """A direct limb kernel exists for the shape (whatever form the convolution is then run in)."""
    return split and ops.conv3x3_split_supported(c1, c2, b, h, w, cout)


def conv3_route(split: bool, c1: int, c2: int, b: int, h: int, w: int, cout: int, planes: bool = False,
                wino=wino_wanted) -> str:
    """Forward route of a 3x3 stride-1 pad-1 convolution of [b, h, w, c1 (+ c2)] to ``cout`` channels; its data gradient
    is the same question asked of the transposed shape (c1 = the convolution's cout, c2 = 0, cout = its cin).
    ``planes``: the input is held as bf16 limb planes, which the Winograd kernels (they transform fp32 input
    themselves) cannot read."""
    if split and not planes and wino(c1, c2, b, h, w, cout):
        return WINO
    if limb_takes(split, c1, c2, b, h, w, cout):
        return LIMB
    return TILE


def wgrad_route(split: bool, cout: int, c1: int, c2: int, b: int, h: int, w: int, planes: bool) -> str:
    """Weight-gradient route of the same convolution ([b, h, w] = the output gradient's map)."""
    if split and not planes and ops.conv3x3_wgrad_wino_wanted(cout, c1, c2, b, h, w):
        return WINO
    if split and ops.conv3x3_wgrad_split_supported(cout, c1, b, h, w) and \
            (c2 == 0 or ops.conv3x3_wgrad_split_supported(cout, c2, b, h, w)):
        return LIMB
    return NONE if c2 else TILE


def pointwise_route(split: bool, k1: int, k2: int, m: int, n: int) -> str:
    """Route of a pointwise contraction y[m][n] = [a1 | a2][m][k1 + k2] @ B^T - a 1x1 convolution, a NIN projection, the
    stride-2 pyramid GEMM, forward or data gradient (then with the channel roles swapped).  The ONE place that asks
    ops.gemm_split_supported / ops.gemm_tail_supported for the executor's GEMMs."""
    if split and ops.gemm_split_supported(k1, k2, m, n):
        return LIMB
    if split and k2 == 0 and ops.gemm_tail_supported(k1, m, n):
        return LIMB_TAIL
    return TILE


def pointwise_wgrad_route(split: bool, m: int, n: int, n2: int, k: int) -> str:
    """Route of a pointwise weight gradient dW[m][n + n2] = A[k][m]^T [B | B2][k][n + n2] (k = pixels).  The ONE place that
    asks ops.gemm_tn_split_supported / ops.gemm_tn_split_tail_supported for the executor's 1x1 / NIN weight gradients."""
    if split and ops.gemm_tn_split_supported(m, n, k) and n2 % 128 == 0:
        return LIMB
    if split and n2 == 0 and ops.gemm_tn_split_tail_supported(m, n, k):
        return LIMB_TAIL
    return TILE


def batched_route(split: bool, ta: int, tb: int, m: int, n: int, k: int) -> str:
    """Route of a batched activation x activation product c[b] = alpha op(a[b]) op(b[b]) - the attention block's QK^T, PV
    and their gradients where the fused forward kernel does not run.  The ONE place that asks ops.bgemm_split_supported /
    ops.bgemm_split_tail_supported for the executor (which sends operands that are not 16-byte aligned to the tile engine
    whatever the route)."""
    if split and ops.bgemm_split_supported(ta, tb, m, n, k):
        return LIMB
    if split and ops.bgemm_split_tail_supported(ta, tb, m, n, k):
        return LIMB_TAIL
    return TILE


class AttnPlan(NamedTuple):
    """Kernel choices of one attention block over [m = b * hw][c]."""
    route: str                      # every projection and its data gradient (c -> c, and the fused c -> 3c / 3c -> c)
    fused: bool                     # limb routes: q | k | v come from ONE GEMM into one [m][3c] buffer
    wgrad: str                      # a NIN weight gradient dW[c][c], the one-GEMM q | k | v weight gradient dW[c][3c], and
    qkv_wgrad: str                  # whether that one runs (a limb route takes it and the batched slab reduction cuts its
    qkv_one: bool                   # result into the three parameters)


def attn_plan(split: bool, c: int, m: int) -> AttnPlan:
    route = pointwise_route(split, c, 0, m, c)
    fused = route != TILE
    # c -> c, c -> 3c and 3c -> c take the same route: 3c is a multiple of 128 exactly when c is
    assert not fused or pointwise_route(split, c, 0, m, 3 * c) == route == pointwise_route(split, 3 * c, 0, m, c)
    qkv_wgrad = pointwise_wgrad_route(split, c, 3 * c, 0, m)
    return AttnPlan(route, fused, pointwise_wgrad_route(split, c, c, 0, m), qkv_wgrad,
                    fused and qkv_wgrad != TILE and ops.slab_units(c * c, 2, c, 3 * c) > 0)


def pyramid_plan(split: bool, cin: int, cout: int, m: int):
    """(small, limb, fwd, bwd) of the input pyramid's 3x3 stride-2 convolution to [m][cout].  ``small``: few input channels (im2col
    to K = 64 + a tile-engine GEMM); else ``limb``: im2col + pointwise GEMM on limb routes ``fwd`` / ``bwd``; neither: the tile engine."""
    small = cin * 9 <= 64 and cout % 4 == 0
    fwd, bwd = pointwise_route(split, 9 * cin, 0, m, cout), pointwise_route(split, cout, 0, m, 9 * cin)
    return small, not small and cin % 4 == 0 and fwd != TILE and bwd != TILE, fwd, bwd


def head_fewout(cin: int, cout: int) -> bool:
    """The head's 3x3 convolution to a few output channels runs on its own kernel (ops.conv3x3_fewout)."""
    return ops.conv3x3_fewout_supported(cin, cout)


class BlockPlan(NamedTuple):
    """Kernel choices of one residual block (GroupNorm_0 - Conv_0 - GroupNorm_1 - Conv_1)."""
    conv0: str                      # forward routes (WINO_GN: the GroupNorm apply pass runs inside the convolution)
    conv1: str
    lp0: bool                       # the convolution's input is written as bf16 limb planes by GroupNorm's apply pass
    lp1: bool
    part0: bool                     # the forward launch is asked for GroupNorm partial sums of its output
    part1: bool
    wgrad0: Optional[str] = None    # recording passes only: weight-gradient routes ...
    wgrad1: Optional[str] = None
    dgrad0: Tuple[str, ...] = ()    # ... and data-gradient routes; Conv_0's per source of a two-source block
    dgrad1: Optional[str] = None
    shortcut: Optional[str] = None  # the 1x1 shortcut (blocks that have one): pointwise routes of its forward ...
    shortcut_dgrad: Optional[str] = None    # ... and (recording passes) of its one-source data gradient


def block_plan(split: bool, limb_planes: bool, record: bool, dropout: bool, c1: int, c2: int, b: int, h: int, w: int,
               cout: int, up: bool, down: bool, wino=wino_wanted, shortcut: bool = False) -> BlockPlan:
    """``c2``: channels of the second source of an unmaterialised concatenation (0: one source); ``[h, w]``: the block's
    input map - blocks that resample (``up`` / ``down``) do so between GroupNorm_0 and Conv_0, so both convolutions run
    on the output map."""
    resample = up or down
    ho, wo = (h // 2, w // 2) if down else ((h * 2, w * 2) if up else (h, w))
    # Inference forward (no tape): GroupNorm's apply pass + SiLU run inside the Winograd convolution's input staging where
    # that pays - the activated tensor is needed nowhere else.
    # NOTE (behaviour, kept as it is; ADVICE.md lists both): ops.conv3x3_wino_gn_wanted asks ops.conv3x3_wino_wanted WITHOUT
    # split_ok while ``wino`` below passes True, and set_winograd() does not clear conv3x3_wino_gn_wanted's cache - so
    # after a switch to PSLD_WINOGRAD=0 inside one process a shape fused before stays fused.
    fuse0 = not record and not resample and split and ops.conv3x3_wino_gn_wanted(c1, c2, b, h, w, cout)
    fuse1 = not record and split and not dropout and ops.conv3x3_wino_gn_wanted(cout, 0, b, ho, wo, cout)
    # Otherwise the activations go to the 3x3 convolutions as bf16 LIMB PLANES where the direct limb kernels run both the
    # forward and (when there is one) the weight gradient; a convolution in Winograd form transforms fp32 input itself,
    # and blocks that resample between the normalisation and the convolution keep fp32.
    lp0 = not fuse0 and split and limb_planes and not resample and \
        conv3_route(split, c1, c2, b, h, w, cout, wino=wino) == LIMB and \
        (not record or wgrad_route(split, cout, c1, c2, b, h, w, True) == LIMB)
    lp1 = not fuse1 and split and limb_planes and conv3_route(split, cout, 0, b, ho, wo, cout, wino=wino) == LIMB and \
        (not record or wgrad_route(split, cout, cout, 0, b, ho, wo, True) == LIMB)
    conv0 = WINO_GN if fuse0 else conv3_route(split, c1, c2, b, ho, wo, cout, lp0, wino)
    conv1 = WINO_GN if fuse1 else conv3_route(split, cout, 0, b, ho, wo, cout, lp1, wino)
    # the limb kernels (direct and Winograd) leave GroupNorm partial sums wherever a direct limb kernel takes the shape
    part = ops.gn_part_supported(b, ho * wo, cout)
    part0 = limb_takes(split, c1, c2, b, ho, wo, cout) and part
    part1 = limb_takes(split, cout, 0, b, ho, wo, cout) and part
    assert not lp0 or conv0 == LIMB, "limb planes reach a Conv_0 kernel that cannot read them"
    assert not lp1 or conv1 == LIMB, "limb planes reach a Conv_1 kernel that cannot read them"
    sc = pointwise_route(split, c1, c2, b * ho * wo, cout) if shortcut else None
    if not record:
        return BlockPlan(conv0, conv1, lp0, lp1, part0, part1, shortcut=sc)
    wgrad0 = wgrad_route(split, cout, c1, c2, b, ho, wo, lp0)
    wgrad1 = wgrad_route(split, cout, cout, 0, b, ho, wo, lp1)
    dgrad1 = conv3_route(split, cout, 0, b, ho, wo, cout, wino=wino)
    if c2 == 0:
        dgrad0 = (conv3_route(split, cout, 0, b, ho, wo, c1, wino=wino),)
    else:
        # the two sources' shares are slices of ONE fragment buffer: Winograd form when both take it, else the direct
        # kernels (cat_ok admitted the block because they take both)
        both = all(conv3_route(split, cout, 0, b, h, w, c, wino=wino) == WINO for c in (c1, c2))
        dgrad0 = (WINO, WINO) if both else (LIMB, LIMB)
        assert both or all(limb_takes(split, cout, 0, b, h, w, c) for c in (c1, c2)), "no per-source data gradient"
    assert WINO_GN not in (conv0, conv1), "a fused GroupNorm keeps no activation for the tape"
    assert not lp0 or wgrad0 == LIMB, "limb planes reach a Conv_0 weight gradient that cannot read them"
    assert not lp1 or wgrad1 == LIMB, "limb planes reach a Conv_1 weight gradient that cannot read them"
    assert wgrad0 != NONE, "unsupported two-source weight gradient"
    return BlockPlan(conv0, conv1, lp0, lp1, part0, part1, wgrad0, wgrad1, dgrad0, dgrad1, sc,
                     pointwise_route(split, cout, 0, b * ho * wo, c1 + c2) if shortcut else None)


def cat_ok(split: bool, record: bool, c1: int, c2: int, b: int, h: int, w: int, cout: int, up: bool, down: bool,
           has_shortcut: bool, wino=wino_wanted) -> bool:
    """Can a residual block read the concatenation of a c1- and a c2-channel source without it being materialised?  Needs
    the two-source direct limb forward kernels and, when recording, per-source direct limb data gradients (whatever form
    ``block_plan`` then runs them in) and a two-source weight gradient.  On maps below the direct kernels' geometries (4x4)
    the Winograd kernels stand in for them where ``wino`` wants every one of those launches: ``block_plan`` then runs the
    forward, both data gradients and the two-source weight gradient in Winograd form."""
    if not split or up or down or not has_shortcut:
        return False
    m = b * h * w
    cpg = (c1 + c2) // ops.gn_groups(c1 + c2)
    if c1 % 128 or c2 % 128 or c1 % cpg or c2 % cpg or (c1 // 4) > 256 or (c2 // 4) > 256:
        return False
    if h == 4 and w == 4:
        ok = wino(c1, c2, b, h, w, cout) and ops.gemm_split_supported(c1, c2, m, cout)
        if record:
            ok = ok and all(wino(cout, 0, b, h, w, c) and ops.gemm_split_supported(cout, 0, m, c) for c in (c1, c2)) and \
                wgrad_route(split, cout, c1, c2, b, h, w, False) == WINO and ops.gemm_tn_split_supported(cout, c1, m)
        return ok
    ok = limb_takes(split, c1, c2, b, h, w, cout) and ops.gemm_split_supported(c1, c2, m, cout)
    if record:
        ok = ok and all(limb_takes(split, cout, 0, b, h, w, c) and ops.gemm_split_supported(cout, 0, m, c) and
                        wgrad_route(split, cout, c, 0, b, h, w, True) == LIMB for c in (c1, c2)) and \
            ops.gemm_tn_split_supported(cout, c1, m)
    return ok
