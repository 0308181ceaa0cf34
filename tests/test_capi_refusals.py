"""One refusal table for every entry point of the C ABI that validates before it launches, no GPU: per row
an entry point, one change to a descriptor (or argument list) that passes, the return value and what
isr_last_error() must say: it starts with the entry point's message name and holds the row's substrings.
Every call is refused before anything is launched or dereferenced, so the pointers are made-up aligned
addresses.  A second, short table holds descriptors with two faults and pins which is reported first.

An entry is keyed "function" or "function@form": the forms are further passing descriptors of the same
function (a mask epilogue, a shuffled store, ...), so that a row still changes one thing."""
import ctypes
from collections import namedtuple

from image_super_resolution_amd import _lib

BAD_DESC, UNSUPPORTED = -1, -2
P = 0x10000  # aligned, never followed
F3 = ctypes.c_float * 3
I9, I5 = ctypes.c_int32 * 9, ctypes.c_int32 * 5
WS = dict(workspace=P, ws_bytes=1 << 20)
NAN = float("nan")


def V(ha, wa, cs, pad=0, coff=0, data=P):
    """The tightest view that holds an ha x wa region with `cs` channels and a border of `pad`."""
    return _lib.IsrView(data, ha + 2 * pad, wa + 2 * pad, cs, pad, coff)


def mod(v, **kw):
    """A copy of view v with the fields of kw changed."""
    f = {name: getattr(v, name) for name, _ in _lib.IsrView._fields_}
    return _lib.IsrView(**{**f, **kw})


# fn: the exported function less "isr_"; make: descriptor fields -> ctypes object; args: the call's arguments in
# order ("desc" is the descriptor, every other name is looked up in `good`, absent = NULL: the stream); good: the
# descriptor's fields and the call's arguments, all passing; name: how the messages start; sizes: a size query,
# which answers 0 where the launching form answers an error code.
Entry = namedtuple("Entry", "fn make args good name sizes")
ENTRIES = {}


def E(key, cls, args, good, name=None, sizes=False):
    fn = key.split("@")[0]
    names = {f[0] for f in cls._fields_} if cls else ()
    make = (lambda f: cls(**{k: v for k, v in f.items() if k in names})) if cls else None
    ENTRIES[key] = Entry(fn, make, args, good, name or fn, sizes)


DS, DWS = ("desc", "s"), ("desc", "workspace", "ws_bytes", "s")

# ---- the 3x3 conv: one rule set (conv3x3_validate) behind four entry points
G = dict(n=1, h=30, w=60, ha=32, wa=64)  # a grid of 1 x 2 tiles with a ragged edge
CONV = dict(G, cin=64, cout=64, x=V(32, 64, 64, pad=1), y=V(32, 64, 64, data=2 * P), wpack=3 * P, bias=4 * P,
            slope=0.2, s1=1.0, s2=1.0, shuffle=1)
CONV_FORMS = {
    "": CONV,
    "@g32": dict(CONV, cout=32, y=V(32, 64, 32, data=2 * P)),
    "@sub2": dict(CONV, cin=128, x_sub2=1, x=V(64, 128, 32, pad=2)),
    "@mask": dict(CONV, m=V(32, 64, 64, data=5 * P)),
    "@shuffle": dict(CONV, shuffle=2, y=V(64, 128, 16, data=2 * P)),
    "@shuffle_mask": dict(CONV, shuffle=2, y=V(64, 128, 16, data=2 * P), m=V(64, 128, 16, data=5 * P)),
    "@taps": dict(CONV, taps=1),
}
CONV_FNS = {"conv3x3_fwd": DS, "conv3x3_check": ("desc",), "conv3x3_fwd_variant": ("desc", "variant", "s")}
for fn, args in CONV_FNS.items():
    for form, good in CONV_FORMS.items():
        E(fn + form, _lib.IsrConvDesc, args, dict(good, variant=0), "conv3x3")
E("conv3x3_wino_fwd", _lib.IsrConvDesc, DS, dict(CONV, f16=1), "conv3x3")

HEAD = dict(G, cout=64, x=P, x_u8=0, mean=F3(), inv_std=F3(1, 1, 1), y=V(32, 64, 64, data=2 * P), wpack=3 * P,
            bias=4 * P, slope=0.2)
E("head9x9_fwd", _lib.IsrHeadDesc, DS, HEAD, "head9x9")
E("head9x9_fwd@mask", _lib.IsrHeadDesc, DS, dict(HEAD, m=V(32, 64, 64, data=5 * P)), "head9x9")

TAIL = dict(G, cin=64, x=V(32, 64, 64, pad=4), wpack=2 * P, bias=3 * P, y=4 * P, y_u8=0, f16=0)
TAIL_FNS = {"tail9x9_fwd": DS, "tail9x9_fwd_variant": ("desc", "variant", "s"), "tail9x9_segment_rows": ("desc", "cus")}
for fn, args in TAIL_FNS.items():
    E(fn, _lib.IsrTailDesc, args, dict(TAIL, variant=0, cus=256), "tail9x9")

CHAIN = dict(layers=P, kinds=2 * P, nl=5, n=1, ha=32, wa=32, state=3 * P, acquire=0, f16=0)
E("conv_chain", _lib.IsrChainDesc, DS, CHAIN, "conv chain")
E("conv_chain_variant", _lib.IsrChainDesc, ("desc", "variant", "s"), dict(CHAIN, variant=0), "conv chain")

# ---- weight gradients
WGRAD = dict(G, cin=64, cout=64, x=V(32, 64, 64, pad=1), g=V(32, 64, 64, data=2 * P), g_sub2=0, scale=1.0,
             dw=3 * P, db=4 * P, splits=0)
WGRAD_FORMS = {
    "": WGRAD,
    "@x_sub2": dict(WGRAD, cin=128, x_sub2=1, x=V(64, 128, 32, pad=2)),
    "@g_sub2": dict(WGRAD, cout=128, g_sub2=1, g=V(64, 128, 32, data=2 * P)),
}
DVWS = ("desc", "variant", "workspace", "ws_bytes", "s")
WGRAD_FNS = {"wgrad3x3": DWS, "wgrad3x3_partials": DWS, "wgrad3x3_reduce": DWS, "wgrad3x3_variant": DVWS,
             "wgrad3x3_workspace_bytes": ("desc",), "wgrad3x3_variant_workspace_bytes": ("desc", "variant")}
for fn, args in WGRAD_FNS.items():
    for form, good in WGRAD_FORMS.items():
        E(fn + form, _lib.IsrWgradDesc, args, dict(good, variant=0, **WS), "wgrad3x3", sizes=fn.endswith("_bytes"))


def _group(f):
    """The two members m0 and m1 as the array the group entry points take."""
    return (_lib.IsrWgradDesc * 2)(_lib.IsrWgradDesc(**f["m0"]), _lib.IsrWgradDesc(**f["m1"]))


GROUP = dict(m0=WGRAD, m1=dict(WGRAD, cout=32, g=V(32, 64, 32, data=2 * P), dw=5 * P), count=2, variant=0, **WS)
GROUP_FNS = {"wgrad3x3_group": ("desc", "count", "workspace", "ws_bytes", "s"),
             "wgrad3x3_group_variant": ("desc", "count", "variant", "workspace", "ws_bytes", "s"),
             "wgrad3x3_group_workspace_bytes": ("desc", "count")}
for fn, args in GROUP_FNS.items():
    ENTRIES[fn] = Entry(fn, _group, args, GROUP, "wgrad3x3", fn.endswith("_bytes"))

WGRAD9 = dict(G, head=0, p=P, q=V(32, 64, 64, pad=4, data=2 * P), scale=1.0, dw=3 * P, db=4 * P, splits=0)
for fn, args in {"wgrad9x9": DWS, "wgrad9x9_workspace_bytes": ("desc",)}.items():
    E(fn, _lib.IsrWgrad9Desc, args, dict(WGRAD9, **WS), "wgrad9x9", sizes=fn.endswith("_bytes"))
    E(fn + "@head", _lib.IsrWgrad9Desc, args, dict(WGRAD9, head=1, q=V(32, 64, 64, data=2 * P), **WS), "wgrad9x9",
      sizes=fn.endswith("_bytes"))

# ---- elementwise, layout, pool, BatchNorm
EW = dict(G, c=64, y=V(32, 64, 64), a=V(32, 64, 64, data=2 * P), sa=1.0, sb=1.0, mslope=1.0)
E("ew_combine", _lib.IsrEwDesc, DS, EW, "ew")
E("pixel_shuffle2", _lib.IsrEwDesc, DS, dict(EW, c=16, y=V(32, 64, 16), a=V(16, 32, 64, data=2 * P)))
E("pixel_unshuffle2", _lib.IsrEwDesc, DS, dict(EW, h=15, w=30, ha=16, wa=32, y=V(16, 32, 64), a=V(32, 64, 16, data=2 * P)))
CONVERT = dict(G, c=3, nchw=P, v=V(32, 64, 16, data=2 * P), mslope=1.0)
for fn in ("nchw_to_blocked", "blocked_to_nchw"):
    E(fn, _lib.IsrConvertDesc, DS, CONVERT)
POOL = dict(n=1, h=60, w=120, c=64, hao=32, wao=64, x=V(64, 128, 64), y=V(32, 64, 64, data=2 * P), mslope=0.0)
E("maxpool2_fwd", _lib.IsrPoolDesc, DS, POOL, "maxpool2")
E("maxpool2_bwd", _lib.IsrPoolDesc, DS, dict(POOL, g=V(64, 128, 64, data=3 * P)), "maxpool2")
BN = dict(G, c=64, z=V(32, 64, 64), y=V(32, 64, 64, data=2 * P), s1=1.0, s2=1.0, slope=1.0, gamma=3 * P, beta=4 * P,
          running_mean=5 * P, running_var=6 * P, momentum=0.1, eps=1e-5, acc=7 * P, save=8 * P, dgamma=9 * P,
          dbeta=10 * P, gscale=1.0)
BN_FNS = ("bn_stats", "bn_finalize", "bn_apply", "bn_bwd_reduce", "bn_bwd_apply")
for fn in BN_FNS:
    E(fn, _lib.IsrBnDesc, DS, BN, "bn")
E("sr_transform", _lib.IsrSrTransformDesc, DS,
  dict(crops=P, hr=2 * P, lr=3 * P, n=2, t=48, scale=2, hr_norm=0, mean=F3(0.5, 0.5, 0.5), std=F3(0.25, 0.25, 0.25)))

# ---- weight packs: plain arguments
PACK = ("w", "packed", "cout", "cin", "s")
for fn in ("pack_conv3x3", "pack_conv3x3_f16", "pack_conv3x3_wino_f16"):
    E(fn, None, PACK, dict(w=P, packed=2 * P, cout=64, cin=64))
E("pack_conv3x3_dgrad", None, ("w", "packed", "cout", "cin", "scale", "sub2", "s"),
  dict(w=P, packed=2 * P, cout=64, cin=64, scale=1.0, sub2=0))
for fn in ("pack_head9x9", "pack_head9x9_f16"):
    E(fn, None, PACK, dict(w=P, packed=2 * P, cout=64, cin=3), "pack_head9x9")
for fn in ("pack_tail9x9", "pack_tail9x9_f16"):
    E(fn, None, PACK, dict(w=P, packed=2 * P, cout=3, cin=64), "pack_tail9x9")
E("pack_conv3x3_batch", None, ("items", "count", "s"), dict(items=P, count=3))

# ---- multi-tensor optimiser ops: tensor and chunk tables (the descriptor of the Adam forms is isr_adam_args)
MT = dict(ts=P, cs=2 * P, nchunks=4)
ADAM = dict(MT, step=-1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, bc2_sqrt=0.5)
E("mt_adam", _lib.IsrAdamArgs, ("ts", "cs", "nchunks", "desc", "scale", "s"), ADAM)
E("mt_adam_guarded", _lib.IsrAdamArgs, ("ts", "cs", "nchunks", "desc", "scale", "guard", "s"), ADAM, "mt_adam")
E("mt_sumsq", None, ("ts", "cs", "nchunks", "partial", "s"), dict(MT, partial=3 * P))
E("mt_scale", None, ("ts", "cs", "nchunks", "coef", "s"), dict(MT, coef=3 * P))
E("mt_lerp", None, ("ts", "cs", "nchunks", "d", "s"), dict(MT, d=0.999))
E("mt_lerp_guarded", None, ("ts", "cs", "nchunks", "d", "guard", "s"), dict(MT, d=0.999), "mt_lerp")
E("clip_coef", None, ("partial", "count", "max_norm", "out", "s"), dict(partial=P, count=4, max_norm=10.0, out=2 * P))

# ---- uint8 batches, metrics, video frames, dihedral transforms
E("jpeg_roundtrip", _lib.IsrJpegDesc, DWS, dict(n=2, h=32, w=48, src=P, dst=2 * P, quality=3 * P, **WS))
E("jpeg_roundtrip_workspace_bytes", _lib.IsrJpegDesc, ("desc",), dict(n=2, h=32, w=48), "jpeg_roundtrip", sizes=True)
E("hls_l_moments", _lib.IsrHlsMomentsDesc, DS, dict(n=1, h=8, w=8, src=P, out=2 * P, partials=3 * P))
E("iso_noise", _lib.IsrIsoNoiseDesc, DS,
  dict(n=1, h=8, w=8, src=P, dst=2 * P, lum_noise=3 * P, hue_noise=4 * P, apply=5 * P))
E("resample_u8", _lib.IsrResampleDesc, DS,
  dict(n=2, in_h=48, in_w=48, out_h=12, out_w=12, nf=1, ksize_x=17, ksize_y=17, src=P, bounds_x=P, coeffs_x=P,
       bounds_y=P, coeffs_y=P, filter_id=None, dst_u8=2 * P, lr_f32=None, hr_f32=None, hr_norm=0,
       mean=F3(0.5, 0.5, 0.5), std=F3(0.25, 0.25, 0.25)))
E("blur_u8", _lib.IsrBlurDesc, DS, dict(n=2, h=16, w=16, src=P, dst=2 * P, ksize=3 * P, median=4 * P, taps=5 * P))
METRICS = dict(n=2, h=75, w=43, border=4, a=P, b=P, a_u8=1, b_u8=1, a_scale=F3(1, 1, 1), a_shift=F3(),
               b_scale=F3(1, 1, 1), b_shift=F3(), clamp=1, quantize=0, out=P)
E("image_metrics", _lib.IsrMetricsDesc, DWS, dict(METRICS, **WS))
E("image_metrics_workspace_bytes", _lib.IsrMetricsDesc, ("desc",), dict(METRICS, a=None, b=None, out=None),
  "image_metrics", sizes=True)
YUV = dict(n=1, h=4, w=4, layout=0, siting=0, full_range=0, fwd=I9(), inv=I5(), src=P, dst=2 * P)
YUV_FNS = ("yuv420_to_rgb_u8", "rgb_to_yuv420_u8")
for fn in YUV_FNS:
    E(fn, _lib.IsrYuvDesc, DS, YUV)
U16, NORM, TANH = 0, 1, 2  # ISR_RGB_*
YUV16 = dict(YUV, depth=10, shift=0, rgb_kind=U16, mean=F3(), inv_std=F3())
YUV16_FNS = ("yuv420_to_rgb_16", "rgb_to_yuv420_16")
for fn in YUV16_FNS:
    E(fn, _lib.IsrYuv16Desc, DS, YUV16)
E("dihedral", _lib.IsrDihedralDesc, DS, dict(n=2, c=3, h=16, w=24, elem=1, op=1, ops=None, x=P, y=2 * P))
E("ensemble_expand_u8", _lib.IsrEnsembleExpandDesc, DS, dict(n=2, h=16, w=24, x=P, even=2 * P, odd=3 * P))
E("ensemble_reduce", _lib.IsrEnsembleReduceDesc, DS, dict(n=2, h=16, w=24, even=P, odd=2 * P, y=3 * P, y_u8=1))
E("tuning_chain_knobs", None, ("a", "b", "c", "d"), dict(a=0, b=0, c=0, d=0), "chain knobs")
E("tuning_tail_stamps", None, ("buf",), dict(buf=None), "tail stamps")
for fn, name in (("tuning_trunk_knobs", "trunk knobs"),):
    E(fn, None, ("a", "b", "c", "d"), dict(a=0, b=0, c=0, d=0), name)
for fn, name in (("tuning_trunk_item_stamps", "trunk item stamps"), ("tuning_trunk_stamps", "trunk stamps"),
                 ("tuning_conv_stamps", "conv stamps")):
    E(fn, None, ("buf",), dict(buf=None), name)


# ---- rows shared by the entry points of one rule set: (change, return code, substrings)
def view_rows(field, label, v, halo=0, optional=False):
    """Every rule of a view (`v` passes, tightly): present unless optional, the halo, the extent, the channel
    slice, the 16-channel blocking and the alignment."""
    rows = [] if optional else [({field: mod(v, data=None)}, BAD_DESC, (label, "null data"))]
    if halo:
        rows.append(({field: mod(v, pad=halo - 1)}, BAD_DESC, (label, f"halo {halo}")))
    return rows + [
        ({field: mod(v, hp=v.hp - 1)}, BAD_DESC, (label, "smaller than computed region")),
        ({field: mod(v, wp=v.wp - 1)}, BAD_DESC, (label, "smaller than computed region")),
        ({field: mod(v, coff=-16)}, BAD_DESC, (label, "exceed stride")),
        ({field: mod(v, cs=v.cs - 16)}, BAD_DESC, (label, "exceed stride")),
        ({field: mod(v, cs=v.cs + 8)}, BAD_DESC, (label, "multiples of 16")),
        ({field: mod(v, data=v.data + 8)}, BAD_DESC, (label, "16-byte aligned")),
    ]


def tile_grid_rows(empty="empty problem"):
    """n, h, w > 0; ha / wa multiples of the 32 x 32 tile that cover h / w (on the grid G)."""
    return [({"n": 0}, BAD_DESC, (empty,)), ({"h": 0}, BAD_DESC, (empty,)), ({"w": -1}, BAD_DESC, (empty,)),
            ({"ha": 40}, BAD_DESC, ("computed region",)), ({"wa": 80}, BAD_DESC, ("computed region",)),
            ({"h": 40}, BAD_DESC, ("computed region",)), ({"w": 70}, BAD_DESC, ("computed region",))]


def for_each(entries, rows):
    return [(e, *r) for e in entries for r in rows]


Y64, Y16 = V(32, 64, 64, data=6 * P), V(64, 128, 16, data=6 * P)
CONV_ROWS = {
    "": [(None, BAD_DESC, ("null descriptor",)), *tile_grid_rows(),
         ({"cin": 40}, UNSUPPORTED, ("cin 40", "multiple of 16")), ({"cin": 0}, UNSUPPORTED, ("cin 0",)),
         ({"cout": 48}, UNSUPPORTED, ("cout 48", "multiple of 32")), ({"cout": 0}, UNSUPPORTED, ("cout 0",)),
         ({"wpack": None}, BAD_DESC, ("null weights",)),
         ({"shuffle": 0}, UNSUPPORTED, ("shuffle",)), ({"shuffle": 3}, UNSUPPORTED, ("shuffle",)),
         ({"taps": -1}, UNSUPPORTED, ("taps",)), ({"taps": 3}, UNSUPPORTED, ("taps",)),
         *view_rows("x", "conv3x3.x", CONV["x"], halo=1), *view_rows("y", "conv3x3.y", CONV["y"]),
         *view_rows("y2", "conv3x3.y2", Y64, optional=True), *view_rows("r1", "conv3x3.r1", Y64, optional=True),
         *view_rows("r2", "conv3x3.r2", Y64, optional=True),
         ({"r1_cn": 16}, BAD_DESC, ("r1_cn 16",)), ({"r1_cn": -32}, BAD_DESC, ("r1_cn -32",)),
         ({"bias": 4 * P + 4}, BAD_DESC, ("bias", "16-byte aligned")),
         ({"f16": 2}, BAD_DESC, ("f16 must be 0 or 1",)), ({"f16": -1}, BAD_DESC, ("f16 must be 0 or 1",))],
    "@g32": [({"taps": 1}, UNSUPPORTED, ("tap window", "cout % 64")),
             ({"shuffle": 2}, UNSUPPORTED, ("pixel shuffle", "cout % 64"))],
    "@sub2": [({"cin": 64}, UNSUPPORTED, ("x_sub2", "cin % 128", "got 64")),
              ({"shuffle": 2}, UNSUPPORTED, ("x_sub2 with a shuffled store",)),
              *view_rows("x", "conv3x3.x", CONV_FORMS["@sub2"]["x"], halo=2),
              ({"f16": 1}, UNSUPPORTED, ("forward-only",))],
    "@mask": [({"y2": Y64}, UNSUPPORTED, ("mask epilogue takes no second output",)),
              ({"m_c0": 16}, BAD_DESC, ("m_c0 16",)), ({"m_c0": -32}, BAD_DESC, ("m_c0 -32",)),
              *view_rows("m", "conv3x3.m", CONV_FORMS["@mask"]["m"], optional=True),
              ({"f16": 1}, UNSUPPORTED, ("forward-only",))],
    "@shuffle": [({"r1": Y16}, UNSUPPORTED, ("pixel shuffle store takes no residual",)),
                 ({"r2": Y16}, UNSUPPORTED, ("pixel shuffle store takes no residual",)),
                 ({"y2": Y16}, UNSUPPORTED, ("pixel shuffle store takes no residual",)),
                 *view_rows("y", "conv3x3.y", CONV_FORMS["@shuffle"]["y"])],
    "@shuffle_mask": [({"m_c0": 32}, UNSUPPORTED, ("masks all channels",)),
                      *view_rows("m", "conv3x3.m", CONV_FORMS["@shuffle_mask"]["m"], optional=True)],
    "@taps": [({"f16": 1}, UNSUPPORTED, ("forward-only",))],
}
TAIL_ROWS = [(None, BAD_DESC, ("null descriptor",)), *tile_grid_rows("empty"),
             ({"cin": 32}, UNSUPPORTED, ("cin",)), ({"y": None}, BAD_DESC, ("null",)),
             ({"wpack": None}, BAD_DESC, ("null",)), *view_rows("x", "tail9x9.x", TAIL["x"], halo=4),
             ({"x": V(32, 64, 64, pad=1)}, BAD_DESC, ("halo",)), ({"f16": 2}, BAD_DESC, ("f16",))]
WGRAD_ROWS = {
    "": [(None, BAD_DESC, ("null descriptor",)), *tile_grid_rows("empty problem"),
         ({"cin": 48}, UNSUPPORTED, ("cin 48", "multiples of 32")), ({"cout": 16}, UNSUPPORTED, ("cout 16",)),
         ({"cin": 0}, UNSUPPORTED, ("cin 0",)), ({"dw": None}, BAD_DESC, ("null dw",)),
         ({"splits": -1}, BAD_DESC, ("negative split count",)),
         ({"taps": 2}, UNSUPPORTED, ("taps must be 0 or 1",)), ({"taps": -1}, UNSUPPORTED, ("taps must be 0 or 1",)),
         *view_rows("x", "wgrad3x3.x", WGRAD["x"], halo=1), *view_rows("g", "wgrad3x3.g", WGRAD["g"])],
    "@x_sub2": [({"cin": 64}, UNSUPPORTED, ("x_sub2", "cin % 128", "got 64")),
                ({"g_sub2": 1}, UNSUPPORTED, ("x_sub2 with g_sub2",)),
                *view_rows("x", "wgrad3x3.x", WGRAD_FORMS["@x_sub2"]["x"], halo=2)],
    "@g_sub2": [({"cout": 64}, UNSUPPORTED, ("g_sub2", "cout % 128")),
                *view_rows("g", "wgrad3x3.g", WGRAD_FORMS["@g_sub2"]["g"])],
}
GROUP_ROWS = [(None, BAD_DESC, ("group", "null descriptors or n not in [1, 5]")),
              ({"count": 0}, BAD_DESC, ("group", "n not in [1, 5]")), ({"count": 6}, BAD_DESC, ("group", "n not in [1, 5]")),
              ({"m0.dw": None}, BAD_DESC, ("null dw",)), ({"m1.cin": 48}, UNSUPPORTED, ("cin 48",)),
              ({"m1.x": mod(WGRAD["x"], pad=0)}, BAD_DESC, ("wgrad3x3.x", "halo 1")),
              ({"m1.taps": 1}, UNSUPPORTED, ("group", "member 1")), ({"m1.n": 2}, UNSUPPORTED, ("group", "member 1")),
              ({"m0.taps": 1}, UNSUPPORTED, ("group", "member 0"))]
WGRAD9_ROWS = [(None, BAD_DESC, ("null descriptor",)), *tile_grid_rows("empty problem"),
               ({"p": None}, BAD_DESC, ("null p / dw",)), ({"dw": None}, BAD_DESC, ("null p / dw",)),
               ({"splits": -1}, BAD_DESC, ("negative split count",))]
NULL_WS = ({"workspace": None}, BAD_DESC, ("null workspace",))
SMALL_WS = ({"ws_bytes": 16}, BAD_DESC, ("workspace of 16 bytes is smaller than",))
Z64 = V(32, 64, 64, data=11 * P)
BN_COMMON = [(None, BAD_DESC, ("null descriptor",)), ({"n": 0}, BAD_DESC, ("bad problem",)),
             ({"h": 0}, BAD_DESC, ("bad problem",)), ({"w": 0}, BAD_DESC, ("bad problem",)),
             ({"c": 0}, BAD_DESC, ("bad problem",)), ({"c": 24}, BAD_DESC, ("bad problem", "c=24")),
             ({"c": 1040}, BAD_DESC, ("bad problem", "c <= 1024")),
             ({"ha": 16}, BAD_DESC, ("computed region smaller than valid",)),
             ({"wa": 32}, BAD_DESC, ("computed region smaller than valid",)),
             ({"acc": None}, BAD_DESC, ("null acc / save",)), ({"save": None}, BAD_DESC, ("null acc / save",))]
CONVERT_ROWS = [(None, BAD_DESC, ("null descriptor",)), ({"n": 0}, BAD_DESC, ("problem",)),
                ({"h": 0}, BAD_DESC, ("problem",)), ({"w": 0}, BAD_DESC, ("problem",)),
                ({"c": 0}, BAD_DESC, ("problem",)),
                ({"ha": 16}, BAD_DESC, ("computed region smaller than valid",)),
                ({"wa": 32}, BAD_DESC, ("computed region smaller than valid",)),
                ({"nchw": None}, BAD_DESC, ("null nchw pointer",)),
                *view_rows("v", "", CONVERT["v"]), *view_rows("m", "", V(32, 64, 16, data=3 * P), optional=True)]
POOL_ROWS = [(None, BAD_DESC, ("null descriptor",)), ({"n": 0}, BAD_DESC, ("bad problem",)),
             ({"h": 1}, BAD_DESC, ("bad problem",)), ({"w": 1}, BAD_DESC, ("bad problem",)),
             ({"c": 0}, BAD_DESC, ("bad problem",)), ({"c": 24}, BAD_DESC, ("bad problem", "c=24")),
             ({"hao": 16}, BAD_DESC, ("output region too small",)), ({"wao": 32}, BAD_DESC, ("output region too small",)),
             *view_rows("x", "maxpool2.x", POOL["x"]), *view_rows("y", "maxpool2.y", POOL["y"])]
PACK3_ROWS = [({"w": None}, BAD_DESC, ("null pointer",)), ({"packed": None}, BAD_DESC, ("null pointer",)),
              ({"cin": 40}, UNSUPPORTED, ("cin 40", "multiple of 16")), ({"cin": 0}, UNSUPPORTED, ("cin 0",)),
              ({"cout": 48}, UNSUPPORTED, ("cout 48", "multiple of 32")), ({"cout": 0}, UNSUPPORTED, ("cout 0",))]
MT_ROWS = [({"ts": None}, BAD_DESC, ("null tensor / chunk table",)), ({"cs": None}, BAD_DESC, ("null tensor / chunk table",)),
           ({"nchunks": 0}, BAD_DESC, ("bad chunk count 0",)), ({"nchunks": -1}, BAD_DESC, ("bad chunk count -1",)),
           ({"nchunks": (1 << 30) + 1}, BAD_DESC, ("bad chunk count",))]
ADAM_ROWS = [*MT_ROWS, (None, BAD_DESC, ("null args",)), ({"bc2_sqrt": 0.0}, BAD_DESC, ("bad betas / bias correction",)),
             ({"bc2_sqrt": NAN}, BAD_DESC, ("bad betas",)), ({"beta1": 1.0}, BAD_DESC, ("bad betas",)),
             ({"beta1": -0.1}, BAD_DESC, ("bad betas",)), ({"beta2": 1.0}, BAD_DESC, ("bad betas",)),
             ({"beta2": NAN}, BAD_DESC, ("bad betas",))]
YUV_ROWS = [(None, BAD_DESC, ("null descriptor",)), ({"h": 5}, BAD_DESC, ("even",)), ({"w": 3}, BAD_DESC, ("even",)),
            ({"h": 0}, BAD_DESC, ()), ({"w": 0}, BAD_DESC, ()), ({"n": 0}, BAD_DESC, ("batch",)),
            ({"n": 65536}, BAD_DESC, ("batch",)), ({"src": None}, BAD_DESC, ("null",)), ({"dst": None}, BAD_DESC, ("null",)),
            ({"dst": P}, BAD_DESC, ("dst must not be src",)), ({"layout": 2}, UNSUPPORTED, ("layout",)),
            ({"siting": -1}, UNSUPPORTED, ("siting",)), ({"siting": 2}, UNSUPPORTED, ("siting",)),
            ({"h": 32768, "w": 16384}, UNSUPPORTED, ("2^28",))]
YUV16_ROWS = [*YUV_ROWS, ({"rgb_kind": 3}, UNSUPPORTED, ("rgb_kind",)), ({"rgb_kind": -1}, UNSUPPORTED, ("rgb_kind",)),
              ({"depth": 8}, UNSUPPORTED, ("depth",)), ({"depth": 12}, UNSUPPORTED, ("depth",)),
              ({"depth": 16}, UNSUPPORTED, ("depth",)), ({"shift": 7}, UNSUPPORTED, ("shift",)),
              ({"shift": -1}, UNSUPPORTED, ("shift",)), ({"shift": 16}, UNSUPPORTED, ("shift",)),
              ({"src": P + 1}, BAD_DESC, ("aligned",)), ({"dst": 2 * P + 1}, BAD_DESC, ("aligned",)),
              ({"src": P + 3, "dst": 2 * P + 5}, BAD_DESC, ("aligned",))]
REMOVED = ("removed", "DESIGN.md")

# (entry, change (None: a null descriptor; a dotted key reaches into a group's member), return code,
#  further substrings of the message (None: the message is not looked at))
TABLE = [
    *[row for form, rows in CONV_ROWS.items() for row in for_each([fn + form for fn in CONV_FNS], rows)],
    ("conv3x3_fwd_variant", {"variant": 42}, UNSUPPORTED, ("variant 42 not available", "cout 64 / cin 64")),
    ("conv3x3_fwd_variant", {"variant": -1}, UNSUPPORTED, ("variant -1 not available",)),
    ("conv3x3_wino_fwd", None, BAD_DESC, ("conv3x3_wino", "null descriptor")),
    ("conv3x3_wino_fwd", {"f16": 0}, UNSUPPORTED, ("conv3x3_wino", "f16 must be 1")),
    ("conv3x3_wino_fwd", {"shuffle": 2}, UNSUPPORTED, ("conv3x3_wino", "shuffle must be 1")),
    ("conv3x3_wino_fwd", {"m": Y64}, UNSUPPORTED, ("conv3x3_wino", "mask")),
    ("conv3x3_wino_fwd", {"x_sub2": 1}, UNSUPPORTED, ("conv3x3_wino", "x_sub2")),
    ("conv3x3_wino_fwd", {"taps": 1}, UNSUPPORTED, ("conv3x3_wino", "taps")),
    # past its own checks the direct form's rules apply
    ("conv3x3_wino_fwd", {"cin": 40}, UNSUPPORTED, ("multiple of 16",)),
    ("conv3x3_wino_fwd", {"wpack": None}, BAD_DESC, ("null weights",)),
    ("conv3x3_wino_fwd", {"x": mod(CONV["x"], data=None)}, BAD_DESC, ("conv3x3.x", "null data")),
    ("conv3x3_wino_fwd", {"ha": 40}, BAD_DESC, ("computed region",)),
    ("head9x9_fwd", None, BAD_DESC, ("null descriptor",)),
    *for_each(["head9x9_fwd"], tile_grid_rows("empty problem")),
    ("head9x9_fwd", {"cout": 32}, UNSUPPORTED, ("cout must be 64",)),
    ("head9x9_fwd", {"x": None}, BAD_DESC, ("null input or weights",)),
    ("head9x9_fwd", {"wpack": None}, BAD_DESC, ("null input or weights",)),
    *for_each(["head9x9_fwd"], view_rows("y", "head9x9.y", HEAD["y"])),
    *for_each(["head9x9_fwd"], view_rows("y2", "head9x9.y2", Y64, optional=True)),
    *for_each(["head9x9_fwd"], view_rows("m", "head9x9.m", Y64, optional=True)),
    ("head9x9_fwd", {"bias": 4 * P + 8}, BAD_DESC, ("bias", "16-byte aligned")),
    ("head9x9_fwd", {"f16": 2}, BAD_DESC, ("f16 must be 0 or 1",)),
    ("head9x9_fwd@mask", {"f16": 1}, UNSUPPORTED, ("forward-only",)),
    *for_each(TAIL_FNS, TAIL_ROWS),
    *[("tail9x9_fwd_variant", {"variant": v}, UNSUPPORTED, (f"variant {v} ", *REMOVED)) for v in (1, 2, 4, 6, 12, 36, 70, 117)],
    *for_each(["conv_chain", "conv_chain_variant"], [
        (None, BAD_DESC, ("null layers / kinds / state",)), ({"layers": None}, BAD_DESC, ("null layers",)),
        ({"kinds": None}, BAD_DESC, ("kinds",)), ({"state": None}, BAD_DESC, ("state",)),
        ({"nl": 0}, BAD_DESC, ("nl not in [1, 1024]",)), ({"nl": 1025}, BAD_DESC, ("nl not in [1, 1024]",)),
        ({"n": 0}, BAD_DESC, ("bad grid", "n=0")), ({"ha": 0}, BAD_DESC, ("bad grid", "ha=0")),
        ({"ha": 24}, BAD_DESC, ("bad grid", "ha=24")), ({"wa": 48}, BAD_DESC, ("bad grid", "wa=48")),
        ({"wa": 0}, BAD_DESC, ("bad grid",)), ({"f16": 2}, BAD_DESC, ("f16 must be 0 or 1",))]),
    *[("conv_chain_variant", {"variant": v}, UNSUPPORTED, (f"variant {v} ", *REMOVED)) for v in range(1, 10)],
    ("conv_chain", {"n": 1 << 25}, UNSUPPORTED, ("unsupported grid or layer count",)),
    ("tuning_chain_knobs", {}, UNSUPPORTED, REMOVED),
    ("tuning_tail_stamps", {}, UNSUPPORTED, REMOVED),
    *[row for form, rows in WGRAD_ROWS.items() for row in for_each([fn + form for fn in WGRAD_FNS], rows)],
    *for_each(["wgrad3x3", "wgrad3x3_partials", "wgrad3x3_reduce", "wgrad3x3_variant"], [NULL_WS, SMALL_WS]),
    ("wgrad3x3_variant", {"variant": 17}, UNSUPPORTED, ("no variant 17",)),
    ("wgrad3x3_variant", {"variant": -1}, UNSUPPORTED, ("no variant -1",)),
    ("wgrad3x3_variant_workspace_bytes", {"variant": 17}, UNSUPPORTED, None),
    *for_each(GROUP_FNS, GROUP_ROWS),
    *for_each(["wgrad3x3_group", "wgrad3x3_group_variant"], [
        ({"workspace": None}, BAD_DESC, ("group", "null workspace")),
        ({"ws_bytes": 16}, BAD_DESC, ("group", "workspace of 16 bytes is smaller than"))]),
    ("wgrad3x3_group_variant", {"variant": 2}, UNSUPPORTED, ("group", "no variant 2")),
    ("wgrad3x3_group_variant", {"variant": -1}, UNSUPPORTED, ("group", "no variant -1")),
    *for_each(["wgrad9x9", "wgrad9x9@head", "wgrad9x9_workspace_bytes", "wgrad9x9_workspace_bytes@head"], WGRAD9_ROWS),
    *for_each(["wgrad9x9", "wgrad9x9_workspace_bytes"], view_rows("q", "wgrad9x9.q", WGRAD9["q"], halo=4)),
    *for_each(["wgrad9x9@head", "wgrad9x9_workspace_bytes@head"], view_rows("q", "wgrad9x9.q", V(32, 64, 64, data=2 * P))),
    *for_each(["wgrad9x9", "wgrad9x9@head"], [NULL_WS, SMALL_WS]),
    ("ew_combine", None, BAD_DESC, ("ew_combine", "null descriptor")),
    *[("ew_combine", ch, BAD_DESC, ("ew_combine", "bad problem")) for ch in ({"n": 0}, {"h": 0}, {"w": 0}, {"c": 0}, {"c": 24})],
    ("ew_combine", {"ha": 16}, BAD_DESC, ("ew_combine", "computed region smaller than valid")),
    ("ew_combine", {"wa": 32}, BAD_DESC, ("ew_combine", "computed region smaller than valid")),
    *for_each(["ew_combine"], view_rows("y", "ew.y", EW["y"]) + view_rows("a", "ew.a", EW["a"])),
    *for_each(["ew_combine"], view_rows("b", "ew.b", Y64, optional=True) + view_rows("m", "ew.m", Y64, optional=True)),
    ("pixel_shuffle2", None, BAD_DESC, ("null descriptor",)),
    *[("pixel_shuffle2", ch, BAD_DESC, ("bad problem",)) for ch in ({"n": 0}, {"h": 0}, {"w": 0}, {"c": 0}, {"c": 24})],
    ("pixel_shuffle2", {"h": 29}, BAD_DESC, ("output 29x60 must be even",)),
    ("pixel_shuffle2", {"w": 59}, BAD_DESC, ("output 30x59 must be even",)),
    ("pixel_shuffle2", {"ha": 31}, BAD_DESC, ("computed region 31x64 must be even",)),
    ("pixel_shuffle2", {"wa": 63}, BAD_DESC, ("computed region 32x63 must be even",)),
    ("pixel_shuffle2", {"ha": 28}, BAD_DESC, ("computed region", "28x64", "30x60")),
    ("pixel_shuffle2", {"b": Y64}, UNSUPPORTED, ("takes no b / m operand",)),
    ("pixel_shuffle2", {"m": Y64}, UNSUPPORTED, ("takes no b / m operand",)),
    *for_each(["pixel_shuffle2"], view_rows("y", "pixel_shuffle2.y", ENTRIES["pixel_shuffle2"].good["y"])),
    *for_each(["pixel_shuffle2"], view_rows("a", "pixel_shuffle2.a", ENTRIES["pixel_shuffle2"].good["a"])),
    ("pixel_unshuffle2", None, BAD_DESC, ("null descriptor",)),
    *[("pixel_unshuffle2", ch, BAD_DESC, ("bad problem", "c % 64")) for ch in ({"n": 0}, {"h": 0}, {"w": 0}, {"c": 0}, {"c": 32})],
    ("pixel_unshuffle2", {"ha": 8}, BAD_DESC, ("computed region smaller than valid",)),
    ("pixel_unshuffle2", {"wa": 16}, BAD_DESC, ("computed region smaller than valid",)),
    ("pixel_unshuffle2", {"b": Y64}, UNSUPPORTED, ("takes no b operand",)),
    *for_each(["pixel_unshuffle2"], view_rows("y", "pixel_unshuffle2.y", ENTRIES["pixel_unshuffle2"].good["y"])),
    *for_each(["pixel_unshuffle2"], view_rows("a", "pixel_unshuffle2.a", ENTRIES["pixel_unshuffle2"].good["a"])),
    *for_each(["pixel_unshuffle2"], view_rows("m", "pixel_unshuffle2.m", V(32, 64, 16, data=3 * P), optional=True)),
    *for_each(["nchw_to_blocked", "blocked_to_nchw"], CONVERT_ROWS),
    *for_each(["maxpool2_fwd", "maxpool2_bwd"], POOL_ROWS),
    *for_each(["maxpool2_bwd"], view_rows("g", "maxpool2.g", ENTRIES["maxpool2_bwd"].good["g"])),
    *for_each(BN_FNS, BN_COMMON),
    *for_each(["bn_stats", "bn_apply", "bn_bwd_reduce", "bn_bwd_apply"], view_rows("z", "bn.z", BN["z"])),
    *for_each(["bn_apply", "bn_bwd_reduce", "bn_bwd_apply"], view_rows("y", "bn.y", BN["y"])),
    *for_each(["bn_apply"], view_rows("r1", "bn.r1", Z64, optional=True) + view_rows("r2", "bn.r2", Z64, optional=True)),
    *for_each(["bn_bwd_apply"], view_rows("dz", "bn.dz", Z64, optional=True)),
    ("bn_apply", {"gamma": None}, BAD_DESC, ("null gamma / beta",)),
    ("bn_apply", {"beta": None}, BAD_DESC, ("null gamma / beta",)),
    ("bn_bwd_apply", {"gamma": None}, BAD_DESC, ("null gamma / beta",)),
    ("bn_finalize", {"running_mean": None}, BAD_DESC, ("running stats pair",)),
    ("bn_finalize", {"running_var": None}, BAD_DESC, ("running stats pair",)),
    ("sr_transform", None, BAD_DESC, ("null descriptor / buffer",)),
    *[("sr_transform", {k: None}, BAD_DESC, ("null descriptor / buffer",)) for k in ("crops", "hr", "lr")],
    ("sr_transform", {"scale": 1}, UNSUPPORTED, ("scale 1 not in",)),
    ("sr_transform", {"scale": 5}, UNSUPPORTED, ("scale 5 not in",)),
    *[("sr_transform", ch, BAD_DESC, ("bad batch",)) for ch in ({"n": 0}, {"t": 0}, {"t": 49}, {"n": 1 << 20})],
    ("sr_transform", {"std": F3(0.25, 0.0, 0.25)}, BAD_DESC, ("std[1] is zero",)),
    *for_each(["pack_conv3x3", "pack_conv3x3_f16", "pack_conv3x3_wino_f16"], PACK3_ROWS),
    ("pack_conv3x3_dgrad", {"w": None}, BAD_DESC, ("null pointer",)),
    ("pack_conv3x3_dgrad", {"packed": None}, BAD_DESC, ("null pointer",)),
    ("pack_conv3x3_dgrad", {"cin": 48}, UNSUPPORTED, ("cin 48 / cout 64 must be multiples of 32",)),
    ("pack_conv3x3_dgrad", {"cout": 16}, UNSUPPORTED, ("must be multiples of 32",)),
    ("pack_conv3x3_dgrad", {"cin": 0}, UNSUPPORTED, ("must be multiples of 32",)),
    ("pack_conv3x3_dgrad", {"sub2": 1}, UNSUPPORTED, ("sub2 needs cout % 128",)),
    *for_each(["pack_head9x9", "pack_head9x9_f16"], [
        ({"w": None}, BAD_DESC, ("null pointer",)), ({"packed": None}, BAD_DESC, ("null pointer",)),
        ({"cout": 32}, UNSUPPORTED, ("need cout 64", "got 32, 3")), ({"cin": 0}, UNSUPPORTED, ("need cout 64",)),
        ({"cin": 4}, UNSUPPORTED, ("cin <= 3",))]),
    *for_each(["pack_tail9x9", "pack_tail9x9_f16"], [
        ({"w": None}, BAD_DESC, ("null pointer",)), ({"packed": None}, BAD_DESC, ("null pointer",)),
        ({"cout": 4}, UNSUPPORTED, ("need cout 3, cin 64", "got 4, 64")), ({"cin": 32}, UNSUPPORTED, ("need cout 3, cin 64",))]),
    *[("pack_conv3x3_batch", ch, BAD_DESC, ("bad item table",)) for ch in ({"items": None}, {"count": 0}, {"count": 65536})],
    *for_each(["mt_adam", "mt_adam_guarded"], ADAM_ROWS),
    *for_each(["mt_sumsq", "mt_scale", "mt_lerp", "mt_lerp_guarded"], MT_ROWS),
    ("mt_sumsq", {"partial": None}, BAD_DESC, ("null partial buffer",)),
    ("mt_scale", {"coef": None}, BAD_DESC, ("null coefficient",)),
    *[("clip_coef", ch, BAD_DESC, ("bad arguments",)) for ch in ({"partial": None}, {"out": None}, {"count": 0})],
    ("jpeg_roundtrip", None, BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=1, h=24, w=32), UNSUPPORTED, ("16",)),
    ("jpeg_roundtrip", dict(ws_bytes=16), BAD_DESC, ("workspace",)),
    ("jpeg_roundtrip", dict(n=0), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=65536), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(h=0), BAD_DESC, ()),
    ("jpeg_roundtrip", dict(n=1, dst=None), BAD_DESC, ("null",)),
    ("jpeg_roundtrip", dict(n=4, h=16384, w=16384), UNSUPPORTED, ("31 bits",)),
    ("jpeg_roundtrip", dict(src=P + 4), BAD_DESC, ("aligned",)),
    ("jpeg_roundtrip", dict(quality=3 * P + 2), BAD_DESC, ("aligned",)),
    ("jpeg_roundtrip", dict(workspace=None), BAD_DESC, ("workspace",)),
    ("jpeg_roundtrip", dict(workspace=P + 8), BAD_DESC, ("workspace",)),
    ("jpeg_roundtrip_workspace_bytes", None, BAD_DESC, ("null descriptor",)),
    ("jpeg_roundtrip_workspace_bytes", dict(n=1, h=24, w=32), UNSUPPORTED, ("16",)),
    ("jpeg_roundtrip_workspace_bytes", dict(n=0), BAD_DESC, ()),
    ("hls_l_moments", None, BAD_DESC, ()),
    ("hls_l_moments", dict(h=0), BAD_DESC, ()),
    ("hls_l_moments", dict(n=0), BAD_DESC, ()),
    ("hls_l_moments", dict(n=65536), BAD_DESC, ()),
    ("hls_l_moments", dict(partials=None), BAD_DESC, ("null",)),
    ("hls_l_moments", dict(out=2 * P + 4), BAD_DESC, ("aligned",)),
    ("iso_noise", None, BAD_DESC, ()),
    ("iso_noise", dict(hue_noise=None), BAD_DESC, ("null",)),
    ("iso_noise", dict(w=-1), BAD_DESC, ()),
    ("iso_noise", dict(h=0), BAD_DESC, ()),
    ("iso_noise", dict(n=0), BAD_DESC, ()),
    ("iso_noise", dict(n=65536), BAD_DESC, ()),
    ("iso_noise", dict(lum_noise=3 * P + 2), BAD_DESC, ("aligned",)),
    ("iso_noise", dict(h=1 << 20, w=1 << 20), UNSUPPORTED, ("workgroups",)),
    ("resample_u8", None, BAD_DESC, ()),
    ("resample_u8", dict(out_h=13, hr_f32=0x30000), UNSUPPORTED, ("integer ratio",)),
    ("resample_u8", dict(in_w=109), UNSUPPORTED, ("ratio",)),
    ("resample_u8", dict(out_w=0), UNSUPPORTED, ("sizes",)),
    ("resample_u8", dict(in_h=0), UNSUPPORTED, ("sizes",)),
    ("resample_u8", dict(ksize_x=50), UNSUPPORTED, ("ksize",)),
    ("resample_u8", dict(ksize_y=0), UNSUPPORTED, ("ksize",)),
    ("resample_u8", dict(n=4, in_h=16384, in_w=16384, out_h=4096, out_w=4096), UNSUPPORTED, ("31 bits",)),
    ("resample_u8", dict(dst_u8=None), BAD_DESC, ("no output",)),
    ("resample_u8", dict(src=None), BAD_DESC, ("null",)),
    ("resample_u8", dict(coeffs_y=None), BAD_DESC, ("null",)),
    ("resample_u8", dict(nf=0), BAD_DESC, ()),
    ("resample_u8", dict(n=0), BAD_DESC, ()),
    ("resample_u8", dict(n=65536), BAD_DESC, ()),
    ("resample_u8", dict(dst_u8=P), BAD_DESC, ("must not be src",)),
    ("resample_u8", dict(lr_f32=0x30004), BAD_DESC, ("aligned",)),
    ("resample_u8", dict(src=P + 2), BAD_DESC, ("aligned",)),
    ("resample_u8", dict(lr_f32=0x30000, std=F3(0.25, 0.25, 0.0)), BAD_DESC, ("std[2] is zero",)),
    ("blur_u8", None, BAD_DESC, ("null descriptor",)),
    ("blur_u8", dict(h=6), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(w=6), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(h=0), UNSUPPORTED, ("smaller than",)),
    ("blur_u8", dict(n=0), BAD_DESC, ()),
    ("blur_u8", dict(n=-1), BAD_DESC, ()),
    ("blur_u8", dict(n=65536), BAD_DESC, ()),
    ("blur_u8", dict(src=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(dst=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(ksize=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(median=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(taps=None), BAD_DESC, ("null",)),
    ("blur_u8", dict(dst=P), BAD_DESC, ("must not be src",)),
    ("blur_u8", dict(taps=5 * P + 2), BAD_DESC, ("aligned",)),
    ("blur_u8", dict(n=4, h=16384, w=16384), UNSUPPORTED, ("31 bits",)),
    ("image_metrics", None, BAD_DESC, ("null descriptor",)),
    ("image_metrics", dict(n=1, h=64, w=64, a=None, b=None, out=None), BAD_DESC, ("null",)),
    ("image_metrics", dict(n=0, h=64, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=65536, h=64, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=0, w=64), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=64, w=-3), BAD_DESC, ()),
    ("image_metrics", dict(n=1, h=20, w=30, border=5), UNSUPPORTED, ("11-pixel", "window")),
    ("image_metrics", dict(border=-1), BAD_DESC, ("negative border -1",)),
    ("image_metrics", dict(workspace=None, ws_bytes=0), BAD_DESC, ("workspace",)),
    ("image_metrics", dict(ws_bytes=16), BAD_DESC, ("workspace",)),
    ("image_metrics_workspace_bytes", None, BAD_DESC, ("null descriptor",)),
    ("image_metrics_workspace_bytes", dict(n=1, h=20, w=30, border=5), UNSUPPORTED, ("11-pixel", "window")),
    ("image_metrics_workspace_bytes", dict(n=0), BAD_DESC, ()),
    *for_each(YUV_FNS, YUV_ROWS),
    *for_each(YUV16_FNS, YUV16_ROWS),
    ("yuv420_to_rgb_16", dict(rgb_kind=TANH), UNSUPPORTED, ("other direction",)),
    ("yuv420_to_rgb_16", dict(rgb_kind=NORM, dst=2 * P + 2), BAD_DESC, ("4-byte",)),
    ("yuv420_to_rgb_16", dict(rgb_kind=NORM, src=P + 1), BAD_DESC, ("2-byte",)),
    ("rgb_to_yuv420_16", dict(rgb_kind=NORM), UNSUPPORTED, ("other direction",)),
    ("rgb_to_yuv420_16", dict(rgb_kind=TANH, src=P + 2), BAD_DESC, ("4-byte",)),
    ("rgb_to_yuv420_16", dict(rgb_kind=TANH, dst=2 * P + 1), BAD_DESC, ("2-byte",)),
    ("dihedral", None, BAD_DESC, ("null descriptor",)),
    ("dihedral", dict(x=None), BAD_DESC, ("null",)),
    ("dihedral", dict(y=None), BAD_DESC, ("null",)),
    ("dihedral", dict(elem=4, x=P + 2), BAD_DESC, ("aligned",)),
    ("dihedral", dict(elem=4, y=2 * P + 1), BAD_DESC, ("aligned",)),
    ("dihedral", dict(h=16, w=16, ops=3 * P + 2), BAD_DESC, ("aligned",)),
    ("dihedral", dict(y=P), BAD_DESC, ("must not be x",)),
    ("dihedral", dict(n=0), BAD_DESC, ("n=0",)),
    ("dihedral", dict(n=-1), BAD_DESC, ()),
    ("dihedral", dict(n=65536), BAD_DESC, ()),
    ("dihedral", dict(c=0), BAD_DESC, ("c=0",)),
    ("dihedral", dict(c=65536), BAD_DESC, ()),
    ("dihedral", dict(h=0), BAD_DESC, ("smaller than",)),
    ("dihedral", dict(w=-3), BAD_DESC, ("smaller than",)),
    ("dihedral", dict(h=1 << 16, w=1 << 15), UNSUPPORTED, ("31 bits",)),
    ("dihedral", dict(elem=2), UNSUPPORTED, ("elem 2",)),
    ("dihedral", dict(elem=0), UNSUPPORTED, ("elem 0",)),
    ("dihedral", dict(ops=3 * P), UNSUPPORTED, ("square",)),
    ("dihedral", dict(op=8), UNSUPPORTED, ("op 8",)),
    ("dihedral", dict(op=-1), UNSUPPORTED, ("op -1",)),
    ("dihedral", dict(n=65535, c=65535), UNSUPPORTED, ("workgroups",)),
    ("ensemble_expand_u8", None, BAD_DESC, ("null descriptor",)),
    ("ensemble_expand_u8", dict(x=None), BAD_DESC, ("null",)),
    ("ensemble_expand_u8", dict(even=None), BAD_DESC, ("null",)),
    ("ensemble_expand_u8", dict(odd=None), BAD_DESC, ("null",)),
    ("ensemble_expand_u8", dict(even=P), BAD_DESC, ("same buffer",)),
    ("ensemble_expand_u8", dict(odd=2 * P), BAD_DESC, ("same buffer",)),
    ("ensemble_expand_u8", dict(n=0), BAD_DESC, ()),
    ("ensemble_expand_u8", dict(n=16384), BAD_DESC, ("16383",)),
    ("ensemble_expand_u8", dict(w=0), BAD_DESC, ("smaller than",)),
    ("ensemble_expand_u8", dict(h=1 << 16, w=1 << 15), UNSUPPORTED, ("31 bits",)),
    ("ensemble_expand_u8", dict(n=16383, h=32768, w=32768), UNSUPPORTED, ("workgroups",)),
    ("ensemble_reduce", None, BAD_DESC, ("null descriptor",)),
    ("ensemble_reduce", dict(even=None), BAD_DESC, ("null",)),
    ("ensemble_reduce", dict(odd=None), BAD_DESC, ("null",)),
    ("ensemble_reduce", dict(y=None), BAD_DESC, ("null",)),
    ("ensemble_reduce", dict(y=P), BAD_DESC, ("same buffer",)),
    ("ensemble_reduce", dict(odd=P), BAD_DESC, ("same buffer",)),
    ("ensemble_reduce", dict(even=P + 2), BAD_DESC, ("aligned",)),
    ("ensemble_reduce", dict(y_u8=0, y=3 * P + 1), BAD_DESC, ("aligned",)),
    ("ensemble_reduce", dict(n=0), BAD_DESC, ()),
    ("ensemble_reduce", dict(n=16384), BAD_DESC, ("16383",)),
    ("ensemble_reduce", dict(h=0), BAD_DESC, ("smaller than",)),
    ("ensemble_reduce", dict(h=1 << 16, w=1 << 15), UNSUPPORTED, ("31 bits",)),
    ("ensemble_reduce", dict(n=16383, h=32768, w=32768), UNSUPPORTED, ("workgroups",)),
]

# What only a production library refuses: a tuning build (-DISR_TUNING) carries these forms and setters.
PRODUCTION_TABLE = [
    ("wgrad3x3_variant", {"variant": 5}, UNSUPPORTED, ("no variant 5", "-DISR_TUNING")),
    ("wgrad3x3_variant_workspace_bytes", {"variant": 5}, UNSUPPORTED, None),
    ("conv3x3_fwd_variant", {"variant": 1}, UNSUPPORTED, ("variant 1 not available",)),
    ("tuning_trunk_knobs", {}, UNSUPPORTED, ("built without -DISR_TUNING",)),
    ("tuning_trunk_item_stamps", {}, UNSUPPORTED, ("built without -DISR_TUNING",)),
    ("tuning_trunk_stamps", {}, UNSUPPORTED, ("built without -DISR_TUNING",)),
    ("tuning_conv_stamps", {}, UNSUPPORTED, ("built without -DISR_TUNING",)),
]

# Two faults in one descriptor: the first of the two in the order of the checks is the one reported.
ORDER = [
    ("conv3x3_fwd", {"n": 0, "cin": 40}, BAD_DESC, ("empty problem",)),
    ("conv3x3_fwd", {"ha": 40, "cout": 48}, BAD_DESC, ("computed region",)),
    ("conv3x3_fwd", {"cin": 40, "wpack": None}, UNSUPPORTED, ("cin 40",)),
    ("conv3x3_fwd", {"wpack": None, "shuffle": 3}, BAD_DESC, ("null weights",)),
    ("conv3x3_fwd", {"x": mod(CONV["x"], pad=0), "y": mod(CONV["y"], data=None)}, BAD_DESC, ("conv3x3.x",)),
    ("conv3x3_fwd", {"y": mod(CONV["y"], data=None), "f16": 2}, BAD_DESC, ("conv3x3.y",)),
    ("conv3x3_wino_fwd", {"f16": 0, "ha": 40}, UNSUPPORTED, ("conv3x3_wino", "f16")),
    ("head9x9_fwd", {"ha": 40, "cout": 32}, BAD_DESC, ("computed region",)),
    ("tail9x9_fwd", {"cin": 32, "y": None}, UNSUPPORTED, ("cin",)),
    ("wgrad3x3", {"ha": 40, "cin": 48}, BAD_DESC, ("computed region",)),
    ("wgrad3x3", {"dw": None, "workspace": None}, BAD_DESC, ("null dw",)),
    ("wgrad3x3", {"x": mod(WGRAD["x"], pad=0), "g": mod(WGRAD["g"], data=None)}, BAD_DESC, ("wgrad3x3.x",)),
    ("wgrad3x3_variant", {"workspace": None, "variant": 17}, BAD_DESC, ("null workspace",)),
    ("wgrad9x9", {"dw": None, "splits": -1}, BAD_DESC, ("null p / dw",)),
    ("bn_apply", {"c": 24, "ha": 16}, BAD_DESC, ("bad problem",)),
    ("bn_apply", {"ha": 16, "acc": None}, BAD_DESC, ("computed region",)),
    ("bn_apply", {"acc": None, "z": mod(BN["z"], data=None)}, BAD_DESC, ("null acc / save",)),
    ("bn_apply", {"z": mod(BN["z"], data=None), "gamma": None}, BAD_DESC, ("bn.z",)),
    ("yuv420_to_rgb_16", {"dst": P, "n": 0}, BAD_DESC, ("dst must not be src",)),
    ("yuv420_to_rgb_16", {"h": 5, "layout": 2}, BAD_DESC, ("even",)),
    ("yuv420_to_rgb_16", {"layout": 2, "siting": 2}, UNSUPPORTED, ("layout",)),
    ("rgb_to_yuv420_16", {"depth": 8, "rgb_kind": 3}, UNSUPPORTED, ("depth",)),
    ("rgb_to_yuv420_16", {"rgb_kind": NORM, "src": P + 1}, UNSUPPORTED, ("other direction",)),
    ("resample_u8", {"src": None, "n": 0}, BAD_DESC, ("null src",)),
    ("resample_u8", {"n": 0, "in_h": 0}, BAD_DESC, ("bad batch",)),
    ("resample_u8", {"in_h": 0, "ksize_x": 50}, UNSUPPORTED, ("sizes",)),
    ("resample_u8", {"ksize_x": 50, "dst_u8": P}, UNSUPPORTED, ("ksize",)),
]


def _fields(entry, change):
    """The entry's passing values with the row's change applied ("m1.cin" reaches into a group's member)."""
    vals = dict(ENTRIES[entry].good)
    for path, v in (change or {}).items():
        head, _, rest = path.partition(".")
        vals[head] = {**vals[head], rest: v} if rest else v
    return vals


def _call(lib, entry, change):
    """(return value, message) of one row's call."""
    e = ENTRIES[entry]
    vals, args, keep = _fields(entry, change), [], []
    for a in e.args:
        if a != "desc":
            args.append(vals.get(a))
        elif change is None:
            args.append(None)
        else:
            keep.append(e.make({k: v for k, v in vals.items() if k not in e.args}))
            args.append(keep[-1] if isinstance(keep[-1], ctypes.Array) else ctypes.byref(keep[-1]))
    assert lib.isr_resample_ksize(1, 8, 4) > 0 and not lib.isr_last_error()  # no row passes on the last one's message
    rc = getattr(lib, "isr_" + e.fn)(*args)
    return rc, lib.isr_last_error().decode()


def _missed(lib, rows):
    missed = []
    for entry, change, code, says in rows:
        e = ENTRIES[entry]
        rc, msg = _call(lib, entry, change)
        if rc != (0 if e.sizes else code) or (says is not None and not (msg.startswith(e.name) and all(s in msg for s in says))):
            missed.append((entry, change, f"returned {rc}, expected {code}", msg, says))
    return missed


def _is_production(lib):
    d = _lib.IsrWgradDesc(**{k: v for k, v in WGRAD.items()})
    return lib.isr_wgrad3x3_variant_workspace_bytes(ctypes.byref(d), 1) == 0


def test_refused_without_a_launch(built_lib):
    """Every row of the table; all rows that miss are reported together."""
    rows = TABLE + (PRODUCTION_TABLE if _is_production(built_lib) else [])
    missed = _missed(built_lib, rows)
    assert not missed, "\n".join(map(str, missed))
    assert {e for e, *_ in rows} >= set(ENTRIES) - {"tuning_trunk_knobs", "tuning_trunk_item_stamps",
                                                   "tuning_trunk_stamps", "tuning_conv_stamps"}


def test_first_of_two_faults(built_lib):
    missed = _missed(built_lib, ORDER)
    assert not missed, "\n".join(map(str, missed))


def _desc(entry):
    e = ENTRIES[entry]
    return e.make({k: v for k, v in e.good.items() if k not in e.args})


def test_good_descriptors_pass_the_size_queries(built_lib):
    """The table's starting points are not refused themselves, as far as that shows without a launch:
    the check-only and sizing forms validate the same descriptor (pointers apart) and accept it."""
    lib = built_lib
    jpeg = _desc("jpeg_roundtrip")
    assert lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(jpeg)) == 2 * 32 * 48 * 3 // 2
    assert lib.isr_jpeg_roundtrip_workspace_bytes(None) == 0
    assert lib.isr_jpeg_roundtrip_workspace_bytes(ctypes.byref(_lib.IsrJpegDesc(1, 24, 32, P, P, P))) == 0
    metrics = _desc("image_metrics")
    assert lib.isr_image_metrics_workspace_bytes(ctypes.byref(metrics)) > 16
    assert lib.isr_image_metrics_workspace_bytes(None) == 0
    assert lib.isr_image_metrics_workspace_bytes(ctypes.byref(_desc("image_metrics_workspace_bytes"))) > 16
    for form in CONV_FORMS:
        assert lib.isr_conv3x3_check(ctypes.byref(_desc("conv3x3_check" + form))) == 0, (form, lib.isr_last_error())
    wino = _desc("conv3x3_wino_fwd")
    assert lib.isr_conv3x3_check(ctypes.byref(wino)) == 0 and wino.f16 == 1
    for form in WGRAD_FORMS:
        d = _desc("wgrad3x3" + form)
        assert lib.isr_wgrad3x3_workspace_bytes(ctypes.byref(d)) > 16, (form, lib.isr_last_error())
        assert lib.isr_wgrad3x3_variant_workspace_bytes(ctypes.byref(d), 16) > 16, (form, lib.isr_last_error())
    assert lib.isr_wgrad3x3_group_workspace_bytes(_desc("wgrad3x3_group"), 2) > 16, lib.isr_last_error()
    for form in ("", "@head"):
        assert lib.isr_wgrad9x9_workspace_bytes(ctypes.byref(_desc("wgrad9x9" + form))) > 16, (form, lib.isr_last_error())
    # 30 x 60 on 256 CUs: 512 rows halved until they divide ha = 32, then until the CUs have a block each, or 8
    assert lib.isr_tail9x9_segment_rows(ctypes.byref(_desc("tail9x9_segment_rows")), 256) == 8
    assert not lib.isr_last_error()
