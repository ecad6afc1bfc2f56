"""The argument refusals of the C ABI, text and precedence, without a GPU.

A table of calls, each refused before the first HIP call: the return code and the whole lg_last_error() string are compared with
tests/golden/refusals.json.  The other host tests look for a word of the message; this one pins every byte and, through the cases in
which two conditions fail at once, the order of the checks.  Pointers are the constant P (never dereferenced: a refused call has
touched nothing).  `python tests/test_refusals_host.py` records the table from the library LIGHTGAUSSIAN_HIP_LIB names (or the
in-tree one) and refuses a case that does not come back as LG_ERR_INVALID_ARGUMENT."""
import ctypes as C
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightgaussian_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")
P = 0x1000          # a non-null, 16-byte aligned pointer that must never be dereferenced
ODD = 0x1002        # not 4-byte aligned
P4 = 0x1004         # 4-byte but not 16-byte aligned
RAW, JAC, ABS = _lib.FLAG_RAW_PARAMS, _lib.FLAG_SAVE_SH_JACOBIAN, _lib.FLAG_ABSGRAD
LONG_BOTH = _lib.FLAG_LONG_SERIAL | _lib.FLAG_LONG_PARALLEL


def view(W=32, H=32, degree=0, flags=0, seg=0, bg=P, vm=P, pm=P, campos=P):
    return _lib.lg_view(H, W, 1.0, 1.0, bg, 1.0, vm, pm, degree, campos, 0, flags, seg, None)


def gauss(N=10, M=0, means=P, shs=None, colors=P, opac=P, scales=P, rots=P, cov=None, rest=None):
    return _lib.lg_gaussians(N, M, means, shs, colors, opac, scales, rots, cov, rest)


def sh_gauss(**kw):
    return gauss(**{**dict(M=16, shs=P, colors=None), **kw})


def _ref(s):
    return None if s is None else C.byref(s)


# ---- one builder per family of entry points: keyword arguments -> (function name, argument list) ----------------------------------
GRADS = dict(means2D=P, means3D=P, shs=None, colors=P, opacity=P, scales=P, rotations=P, cov3D=None, shs_rest=None)
SH_GRADS = {**GRADS, "shs": P, "colors": None}


def backward(fn="lg_backward", v=view(), g=gauss(), radii=P, geom=P, bin=P, img=P, R=100, dcolor=P, scratch=P, chunks=1, abs_out=P, flagged=True, **grads):
    d = {**GRADS, **grads}
    if fn == "lg_backward_abs" and v is not None and flagged:       # its own view check comes first: the shared cases run behind it
        v = _lib.lg_view.from_buffer_copy(v)
        v.flags |= ABS
    args = [_ref(v), _ref(g), radii, geom, bin, img, R, dcolor] + [d[k] for k in GRADS] + [scratch, None]
    if fn != "lg_backward":
        args += [chunks, _lib.CHUNK_FN(), None]
    if fn == "lg_backward_abs":
        args += [abs_out]
    return fn, args


def backward_features(v=view(), g=gauss(), radii=P, geom=P, bin=P, img=P, R=100, dcolor=P, features=P, Cn=3, dout=P, dalpha=None, dfeatures=P,
                      scratch=P, **grads):
    d = {**GRADS, **grads}
    return "lg_backward_features", ([_ref(v), _ref(g), radii, geom, bin, img, R, dcolor, features, Cn, None, dout, dalpha] + [d[k] for k in GRADS]
                                    + [dfeatures, scratch, None])


def backward_camera(v=view(), g=gauss(), radii=P, geom=P, bin=P, R=100, rows=P, dview=P, dproj=P, dcam=P, scratch=P):
    return "lg_backward_camera", [_ref(v), _ref(g), radii, geom, bin, R, rows, dview, dproj, dcam, scratch, None]


def blend_features(v=view(), N=10, geom=P, bin=P, R=100, features=P, Cn=3, out=P):
    return "lg_blend_features", [_ref(v), N, geom, bin, R, features, Cn, None, out, None, None]


def blend_features_backward(v=view(), N=10, geom=P, bin=P, R=100, dout=P, Cn=3, dfeatures=P, scratch=P):
    return "lg_blend_features_backward", [_ref(v), N, geom, bin, R, dout, Cn, dfeatures, scratch, None]


def _adam_entry(e, numel=16, step=1, ptr=P, **kw):
    e.param, e.grad, e.exp_avg, e.exp_avg_sq = (kw.get(k, ptr) for k in ("param", "grad", "exp_avg", "exp_avg_sq"))
    e.numel, e.lr, e.weight_decay, e.step = numel, 1e-3, 0.0, step


def adam(tensors=(dict(),), n=None, beta1=0.9, beta2=0.999, table=True):
    arr = (_lib.lg_adam_tensor * max(len(tensors), 1))()
    for e, kw in zip(arr, tensors):
        _adam_entry(e, **kw)
    return "lg_adam_step", [len(tensors) if n is None else n, arr if table else None, beta1, beta2, 1e-8, 0, None]


def adam_rows(tensors=(dict(),), n=None, beta1=0.9, beta2=0.999, table=True):
    arr = (_lib.lg_adam_rows_tensor * max(len(tensors), 1))()
    for e, kw in zip(arr, tensors):
        kw = dict(kw)
        e.row_mask, e.rows = kw.pop("mask", 0x2001), kw.pop("rows", 4)
        _adam_entry(e.t, **kw)
    return "lg_adam_step_rows", [len(tensors) if n is None else n, arr if table else None, beta1, beta2, 1e-8, 0, None]


def loss_forward(Cn=3, H=32, W=32, img=P, gt=P, state=P, out=P, flags=0):
    return "lg_loss_forward", [Cn, H, W, img, gt, state, out, flags, None]


def loss_backward(Cn=3, H=32, W=32, img=P, gt=P, state=P, dimg=P, flags=0):
    return "lg_loss_backward", [Cn, H, W, img, gt, state, P, 1.0, P, 1.0, dimg, flags, None]


def sh_grad(N=10, M=16, D=3, V=1, means=P, campos=P, drgb=P, stride=None, divisor=1.0, dshs=P):
    return "lg_sh_grad_from_rgb", [N, M, D, V, means, campos, drgb, 3 * N if stride is None else stride, divisor, 0, dshs, P, None]


def vq_colors(N=10, M=16, D=3, means=P, campos=P, slot=P, rows=P, stride=96, out=P):
    return "lg_vq_colors", [N, M, D, means, campos, slot, rows, stride, out, 0, None]


def vq_colors_bwd(N=10, M=16, D=3, K=4, n_rows=8, means=P, campos=P, slot=P, rows=P, stride=96, drgb=P, index=P, drows=P, scratch=P):
    return "lg_vq_colors_bwd", [N, M, D, K, n_rows, means, campos, slot, rows, stride, drgb, index, drows, P, scratch, 0, None]


def vq_code_index(N=10, K=4, slot=P, index=P, scratch=P):
    return "lg_vq_code_index", [N, K, slot, index, scratch, None]


def vq_ema_step(n=10, d=8, K=4, x=P, embed=P, size=P, out=P, scratch=P):
    return "lg_vq_ema_step", [n, d, K, x, None, embed, size, 0.99, 1e-5, out, scratch, 0, None]


def compact_rows(N=10, dest=P, tensors=((P, P, 12),), n=None, tables=True):
    k = max(len(tensors), 1)
    src, dst, rb = (C.c_void_p * k)(*[t[0] for t in tensors]), (C.c_void_p * k)(*[t[1] for t in tensors]), (C.c_int32 * k)(*[t[2] for t in tensors])
    return "lg_compact_rows", [N, dest, len(tensors) if n is None else n] + ([src, dst, rb] if tables else [None, None, None]) + [None]


def densify_rows(N=10, N_out=12, map_=P, record=P, tensors=(dict(),), n=None, table=True, rotation=P, scaling=P, noise=P, noise_rows=4):
    arr = (_lib.lg_densify_tensor * max(len(tensors), 1))()
    for e, kw in zip(arr, tensors):
        e.src, e.dst, e.row_words, e.role = kw.get("src", P), kw.get("dst", P), kw.get("words", 3), kw.get("role", _lib.DENSIFY_COPY)
    return "lg_densify_rows", [N, N_out, map_, record, len(tensors) if n is None else n, arr if table else None, rotation, scaling, noise,
                               noise_rows, 0, None]


def filter3d_update(N=10, means=P, V=2, cameras=P, filt=P, scratch=P):
    return "lg_filter3d_update", [N, means, V, cameras, filt, None, scratch, 0, None]


def filter3d_apply(N=10, scaling=P, opacity=P, filt=P, out_s=P, out_o=P):
    return "lg_filter3d_apply", [N, scaling, opacity, filt, out_s, out_o, 0, None]


def filter3d_apply_bwd(N=10, scaling=P, opacity=P, filt=P, ds=P, do=P, out_s=P, out_o=P):
    return "lg_filter3d_apply_bwd", [N, scaling, opacity, filt, ds, do, out_s, out_o, 0, None]


# ---- the table ---------------------------------------------------------------------------------------------------------------------
WIDE = 65536 * 16           # 65536 tile columns: "image too large"

# check_args, shared by the four backwards and lg_backward_camera: (id, keyword arguments of the builder)
CHECK_ARGS = [
    ("null_view", dict(v=None)),
    ("null_gaussians", dict(g=None)),
    ("negative_N", dict(g=gauss(N=-1))),
    ("zero_width", dict(v=view(W=0))),
    ("negative_N+bad_segment", dict(g=gauss(N=-1), v=view(seg=100))),
    ("bad_segment_32", dict(v=view(seg=32))),
    ("bad_segment_100", dict(v=view(seg=100))),
    ("bad_segment+long_flags", dict(v=view(seg=100, flags=LONG_BOTH))),
    ("long_flags", dict(v=view(flags=LONG_BOTH))),
    ("long_flags+too_many", dict(v=view(flags=LONG_BOTH), g=gauss(N=1 << 29))),
    ("too_many", dict(g=gauss(N=1 << 29))),
    ("too_many+no_colour_input", dict(g=gauss(N=1 << 29, colors=None))),
    ("no_colour_input", dict(g=gauss(colors=None))),
    ("both_colour_inputs", dict(g=gauss(shs=P, M=16))),
    ("both_colour_inputs+no_covariance", dict(g=gauss(shs=P, M=16, scales=None, rots=None))),
    ("no_covariance", dict(g=gauss(scales=None, rots=None))),
    ("scales_without_rotations", dict(g=gauss(rots=None))),
    ("both_covariances", dict(g=gauss(cov=P))),
    ("rest_without_raw", dict(g=sh_gauss(rest=P))),
    ("rest_without_raw+bad_M", dict(g=sh_gauss(rest=P, M=5))),
    ("raw_with_precomputed_colours", dict(v=view(flags=RAW))),
    ("raw_with_precomputed_covariance", dict(v=view(flags=RAW), g=sh_gauss(scales=None, rots=None, cov=P, rest=P))),
    ("raw_without_rest", dict(v=view(flags=RAW), g=sh_gauss())),
    ("raw_without_rest+bad_M", dict(v=view(flags=RAW), g=sh_gauss(M=5))),
    ("bad_M_0", dict(g=sh_gauss(M=0))),
    ("bad_M_5", dict(g=sh_gauss(M=5))),
    ("bad_M_25", dict(g=sh_gauss(M=25))),
    ("bad_M+bad_degree", dict(g=sh_gauss(M=5), v=view(degree=4))),
    ("negative_degree", dict(g=sh_gauss(), v=view(degree=-1))),
    ("degree_4", dict(g=sh_gauss(), v=view(degree=4))),
    ("degree_2_with_M_4", dict(g=sh_gauss(M=4), v=view(degree=2))),
    ("degree_3_with_M_9", dict(g=sh_gauss(M=9), v=view(degree=3))),
    ("bad_degree+no_bg", dict(g=sh_gauss(M=4), v=view(degree=2, bg=None))),
    ("no_bg", dict(v=view(bg=None))),
    ("no_viewmatrix", dict(v=view(vm=None))),
    ("no_projmatrix", dict(v=view(pm=None))),
    ("no_campos", dict(v=view(campos=None))),
    ("no_means", dict(g=gauss(means=None))),
    ("no_opacities", dict(g=gauss(opac=None))),
    ("no_means+too_large", dict(g=gauss(means=None), v=view(W=WIDE, H=16))),
    ("too_wide", dict(v=view(W=WIDE, H=16))),
    ("too_high", dict(v=view(W=16, H=WIDE))),
]

# backward_impl, behind check_args: the four backwards and lg_backward_features
BACKWARD_IMPL = [
    ("too_large+no_radii", dict(v=view(W=WIDE, H=16), radii=None)),
    ("rest_without_gradient", dict(v=view(flags=RAW), g=sh_gauss(rest=P), **SH_GRADS)),
    ("rest_without_gradient+no_radii", dict(v=view(flags=RAW), g=sh_gauss(rest=P), radii=None, **SH_GRADS)),
    ("rest_gradient_without_shs_gradient", dict(g=sh_gauss(), **{**SH_GRADS, "shs": None, "colors": P, "shs_rest": P})),
    ("rest_gradient_without_shs_gradient+no_radii", dict(g=sh_gauss(), radii=None, **{**SH_GRADS, "shs": None, "colors": P, "shs_rest": P})),
    ("no_radii", dict(radii=None)),
    ("no_geom", dict(geom=None)),
    ("no_binning", dict(bin=None)),
    ("no_img", dict(img=None)),
    ("no_means2D_gradient", dict(means2D=None)),
    ("no_means3D_gradient", dict(means3D=None)),
    ("no_opacity_gradient", dict(opacity=None)),
    ("no_scratch", dict(scratch=None)),
    ("no_scratch+no_colour_gradient", dict(scratch=None, colors=None)),
    ("no_shs_gradient", dict(g=sh_gauss(), **{**SH_GRADS, "shs": None})),
    ("no_colour_gradient", dict(colors=None)),
    ("no_scales_gradient", dict(scales=None)),
    ("no_rotations_gradient", dict(rotations=None)),
    ("no_cov3D_gradient", dict(g=gauss(scales=None, rots=None, cov=P))),
]

FEATURES_ARGS = [
    ("null_view", dict(v=None)),
    ("null_view+bad_C", dict(v=None, Cn=0)),
    ("C_0", dict(Cn=0)),
    ("C_65", dict(Cn=65)),
    ("bad_C+bad_N", dict(Cn=0, N=-1)),
    ("negative_N", dict(N=-1)),
    ("too_many", dict(N=1 << 29)),
    ("bad_N+bad_R", dict(N=-1, R=-1)),
    ("negative_R", dict(R=-1)),
    ("R_2^30", dict(R=1 << 30)),
    ("bad_R+zero_width", dict(R=-1, v=view(W=0))),
    ("zero_width", dict(v=view(W=0))),
    ("zero_height", dict(v=view(H=0))),
    ("zero_width+bad_segment", dict(v=view(W=0, seg=100))),
    ("bad_segment", dict(v=view(seg=100))),
    ("bad_segment+no_geom", dict(v=view(seg=32), geom=None)),
    ("no_geom", dict(geom=None)),
    ("no_geom+no_binning", dict(geom=None, bin=None)),
    ("no_binning", dict(bin=None)),
    ("no_binning+too_large", dict(bin=None, v=view(W=WIDE, H=16))),
    ("too_wide", dict(v=view(W=WIDE, H=16))),
]


def _with_g(kw):
    """features_args cases for lg_backward_features, which takes N inside lg_gaussians"""
    kw = dict(kw)
    if "N" in kw:
        kw["g"] = gauss(N=kw.pop("N"))
    return kw


def _adam_cases(build, rows):
    big = (2 ** 31) * 4096          # 2^31 spans
    cases = [
        ("negative_num_tensors", build(n=-1)),
        ("negative_num_tensors+bad_beta", build(n=-1, beta1=1.0)),
        ("beta1_1", build(beta1=1.0)), ("beta1_negative", build(beta1=-0.1)), ("beta2_1", build(beta2=1.0)), ("beta2_nan", build(beta2=float("nan"))),
        ("bad_beta+no_table", build(beta2=1.0, table=False)),
        ("no_table", build(table=False)),
        ("no_table+would_be_bad_numel", build(tensors=(dict(numel=-1),), table=False)),
        ("negative_numel", build(tensors=(dict(numel=-1),))),
        ("negative_numel+bad_step", build(tensors=(dict(numel=-1, step=0),))),
        ("step_0", build(tensors=(dict(step=0),))),
        ("step_0_of_an_empty_tensor", build(tensors=(dict(numel=0, step=0),))),
        ("step_0+null_param", build(tensors=(dict(step=0, param=None),))),
        ("null_param", build(tensors=(dict(param=None),))), ("null_grad", build(tensors=(dict(grad=None),))),
        ("null_exp_avg", build(tensors=(dict(exp_avg=None),))), ("null_exp_avg_sq", build(tensors=(dict(exp_avg_sq=None),))),
        ("null_grad+misaligned_param", build(tensors=(dict(grad=None, param=ODD),))),
        ("misaligned_param", build(tensors=(dict(param=ODD),))), ("misaligned_exp_avg_sq", build(tensors=(dict(exp_avg_sq=ODD),))),
        ("misaligned+too_many_spans", build(tensors=(dict(param=ODD, numel=big),))),
        ("too_many_spans", build(tensors=(dict(numel=big),))),
        ("second_tensor_null_behind_an_empty_one", build(tensors=(dict(numel=0, param=None), dict(grad=None)))),
        ("first_misaligned+second_negative_numel", build(tensors=(dict(param=ODD), dict(numel=-1)))),
        ("first_ok+second_step_0", build(tensors=(dict(), dict(step=-2)))),
    ]
    if rows:
        cases += [
            ("rows_0", build(tensors=(dict(rows=0),))), ("rows_negative", build(tensors=(dict(rows=-3),))),
            ("rows_0+not_a_multiple", build(tensors=(dict(rows=0, numel=17),))),
            ("not_a_multiple_of_rows", build(tensors=(dict(numel=16, rows=5),))),
            ("not_a_multiple+row_too_long", build(tensors=(dict(numel=2 ** 32 + 1, rows=2),))),
            ("row_too_long", build(tensors=(dict(numel=2 ** 32, rows=1),))),
            ("misaligned+rows_0", build(tensors=(dict(param=ODD, rows=0),))),
            ("too_many_spans+rows_0", build(tensors=(dict(numel=big, rows=0),))),
            ("null_param+rows_0", build(tensors=(dict(param=None, rows=0),))),
            ("dense_entry_then_rows_beyond_numel", build(tensors=(dict(mask=None, rows=0), dict(numel=16, rows=32)))),
            ("first_rows_0+second_negative_numel", build(tensors=(dict(rows=0), dict(numel=-1)))),
        ]
    return cases


def _sh_shape_cases(build, first, second):
    """M in {1, 4, 9, 16}, 0 <= D <= 3, (D + 1)^2 <= M, joined with the caller's other first condition and put before its second"""
    return [("negative_N", build(N=-1)), ("M_0", build(M=0, D=0)), ("M_2", build(M=2, D=0)), ("M_5", build(M=5, D=1)), ("M_25", build(M=25)),
            ("negative_degree", build(D=-1)), ("degree_4", build(D=4)), ("degree_1_with_M_1", build(M=1, D=1)), ("degree_2_with_M_4", build(M=4, D=2)),
            ("degree_3_with_M_9", build(M=9, D=3)), ("bad_M+" + first[0], build(M=5, D=1, **first[1])), ("bad_degree+" + second[0], build(D=4, **second[1]))]


def _cases():
    out = []

    def add(prefix, cases):
        out.extend((prefix + "/" + name, call) for name, call in cases)

    for fn in ("lg_backward", "lg_backward_chunked", "lg_backward_abs"):
        add(fn, [(n, backward(fn, **kw)) for n, kw in CHECK_ARGS + BACKWARD_IMPL])
    add("lg_backward_abs", [
        ("view_without_the_flag", backward("lg_backward_abs", flagged=False)),
        ("view_with_another_flag", backward("lg_backward_abs", v=view(flags=_lib.FLAG_FAST_EXP), flagged=False)),
        ("no_flag+no_abs_output", backward("lg_backward_abs", flagged=False, abs_out=None)),
        ("null_view+no_abs_output", backward("lg_backward_abs", v=None, abs_out=None)),
        ("no_abs_output", backward("lg_backward_abs", abs_out=None)),
        ("no_abs_output_of_an_empty_model", backward("lg_backward_abs", abs_out=None, g=gauss(N=0))),
        ("no_abs_output+no_dcolor", backward("lg_backward_abs", abs_out=None, dcolor=None)),
        ("no_dcolor", backward("lg_backward_abs", dcolor=None)),
        ("no_dcolor+bad_R", backward("lg_backward_abs", dcolor=None, R=-1)),
        ("negative_R", backward("lg_backward_abs", R=-1)), ("R_2^30", backward("lg_backward_abs", R=1 << 30)),
        ("bad_R+null_gaussians", backward("lg_backward_abs", R=-1, g=None)),
    ])
    for fn in ("lg_backward", "lg_backward_chunked"):
        add(fn, [("no_dcolor", backward(fn, dcolor=None)), ("no_dcolor+no_colour_gradient", backward(fn, dcolor=None, colors=None))])
    add("lg_backward_features", [("null_gaussians", backward_features(g=None)), ("null_gaussians+null_view", backward_features(g=None, v=None))])
    add("lg_backward_features", [(n, backward_features(**_with_g(kw))) for n, kw in FEATURES_ARGS])
    add("lg_backward_features", [
        ("no_features", backward_features(features=None)), ("no_features+no_dout", backward_features(features=None, dout=None)),
        ("dfeatures_without_dout", backward_features(dout=None)),
        ("no_geom+no_features", backward_features(geom=None, features=None)),
        ("dfeatures_without_dout+long_flags", backward_features(dout=None, v=view(flags=LONG_BOTH))),
    ])
    add("lg_backward_features/behind_its_own_checks", [(n, backward_features(**kw)) for n, kw in CHECK_ARGS[8:] + BACKWARD_IMPL if "too_" not in n or n == "too_many"])
    add("lg_backward_features", [("no_dcolor_is_fine_but_no_scratch", backward_features(dcolor=None, scratch=None))])
    add("lg_backward_camera", [(n, backward_camera(**kw)) for n, kw in CHECK_ARGS])
    add("lg_backward_camera", [
        ("too_large+no_outputs", backward_camera(v=view(W=WIDE, H=16), dview=None)),
        ("no_dviewmatrix", backward_camera(dview=None)), ("no_dprojmatrix", backward_camera(dproj=None)), ("no_dcampos", backward_camera(dcam=None)),
        ("no_output+no_scratch", backward_camera(dcam=None, scratch=None)),
        ("no_scratch", backward_camera(scratch=None)), ("no_scratch+bad_R", backward_camera(scratch=None, R=-1)),
        ("negative_R", backward_camera(R=-1)), ("R_2^30", backward_camera(R=1 << 30)), ("bad_R+no_radii", backward_camera(R=-1, radii=None)),
        ("no_radii", backward_camera(radii=None)), ("no_geom", backward_camera(geom=None)), ("no_binning", backward_camera(bin=None)),
        ("no_rows", backward_camera(rows=None)), ("no_rows+sh_without_jacobian", backward_camera(rows=None, g=sh_gauss())),
        ("sh_without_jacobian", backward_camera(g=sh_gauss())), ("empty_model_no_scratch", backward_camera(g=gauss(N=0), scratch=None)),
    ])
    add("lg_blend_features", [(n, blend_features(**kw)) for n, kw in FEATURES_ARGS])
    add("lg_blend_features", [("no_out", blend_features(out=None)), ("no_features", blend_features(features=None)),
                              ("too_large+no_out", blend_features(v=view(W=WIDE, H=16), out=None)), ("empty_model_no_out", blend_features(N=0, out=None, features=None))])
    add("lg_blend_features_backward", [(n, blend_features_backward(**kw)) for n, kw in FEATURES_ARGS])
    add("lg_blend_features_backward", [("no_dout", blend_features_backward(dout=None)), ("no_dfeatures", blend_features_backward(dfeatures=None)),
                                       ("no_scratch", blend_features_backward(scratch=None)),
                                       ("too_large+no_scratch", blend_features_backward(v=view(W=WIDE, H=16), scratch=None))])
    add("lg_adam_step", _adam_cases(adam, False))
    add("lg_adam_step_rows", _adam_cases(adam_rows, True))
    for name, build, last in (("lg_loss_forward", loss_forward, "out"), ("lg_loss_backward", loss_backward, "dimg")):
        add(name, [("C_0", build(Cn=0)), ("H_0", build(H=0)), ("W_negative", build(W=-1)), ("C_65536", build(Cn=65536)),
                   ("bad_shape+no_img", build(Cn=0, img=None)), ("no_img", build(img=None)), ("no_gt", build(gt=None)), ("no_state", build(state=None)),
                   ("no_" + last, build(**{last: None})), ("no_img+too_high", build(img=None, H=34 * 65535 + 1)),
                   ("too_high", build(H=34 * 65535 + 1, W=1, Cn=1)), ("too_high_l1_only", build(H=34 * 65535 + 1, W=1, Cn=1, flags=_lib.FLAG_L1_ONLY))])
    add("lg_sh_grad_from_rgb", _sh_shape_cases(sh_grad, ("V_0", dict(V=0)), ("no_means", dict(means=None))))
    add("lg_sh_grad_from_rgb", [("V_0", sh_grad(V=0)), ("negative_N+V_0", sh_grad(N=-1, V=0)), ("no_means", sh_grad(means=None)), ("no_campos", sh_grad(campos=None)),
                                ("no_drgb", sh_grad(drgb=None)), ("no_dshs", sh_grad(dshs=None)), ("short_stride", sh_grad(stride=29)),
                                ("divisor_0", sh_grad(divisor=0.0)), ("divisor_nan", sh_grad(divisor=float("nan"))), ("no_means+short_stride", sh_grad(means=None, stride=0))])
    add("lg_vq_colors", _sh_shape_cases(vq_colors, ("short_stride", dict(stride=16)), ("misaligned_rows", dict(rows=P4))))
    add("lg_vq_colors", [("short_stride", vq_colors(stride=80)), ("stride_not_16", vq_colors(stride=100)), ("misaligned_rows", vq_colors(rows=P4)),
                         ("null_rows_pass_the_alignment", vq_colors(rows=None)), ("misaligned_rows+no_means", vq_colors(rows=P4, means=None)),
                         ("empty_model_bad_stride", vq_colors(N=0, stride=8)),
                         ("no_means", vq_colors(means=None)), ("no_campos", vq_colors(campos=None)), ("no_slot", vq_colors(slot=None)), ("no_out", vq_colors(out=None))])
    add("lg_vq_colors_bwd", _sh_shape_cases(vq_colors_bwd, ("short_stride", dict(stride=16)), ("misaligned_rows", dict(rows=P4))))
    add("lg_vq_colors_bwd", [("N_2^30", vq_colors_bwd(N=1 << 30)), ("K_0", vq_colors_bwd(K=0)), ("K_beyond_2^24", vq_colors_bwd(K=(1 << 24) + 1, n_rows=1 << 25)),
                             ("fewer_rows_than_K", vq_colors_bwd(K=4, n_rows=3)), ("n_rows_2^31", vq_colors_bwd(n_rows=1 << 31)),
                             ("bad_K+short_stride", vq_colors_bwd(K=0, stride=16)),
                             ("short_stride", vq_colors_bwd(stride=80)), ("stride_not_16", vq_colors_bwd(stride=100)), ("misaligned_rows", vq_colors_bwd(rows=P4)),
                             ("misaligned_rows+no_index", vq_colors_bwd(rows=P4, index=None)),
                             ("no_drows", vq_colors_bwd(drows=None)), ("no_index", vq_colors_bwd(index=None)), ("no_scratch", vq_colors_bwd(scratch=None)),
                             ("no_rows", vq_colors_bwd(rows=None)), ("no_means", vq_colors_bwd(means=None)), ("no_campos", vq_colors_bwd(campos=None)),
                             ("no_slot", vq_colors_bwd(slot=None)), ("no_drgb", vq_colors_bwd(drgb=None)), ("empty_model_no_index", vq_colors_bwd(N=0, index=None, means=None))])
    add("lg_vq_code_index", [("negative_N", vq_code_index(N=-1)), ("N_2^30", vq_code_index(N=1 << 30)), ("K_0", vq_code_index(K=0)),
                             ("K_beyond_2^24", vq_code_index(K=(1 << 24) + 1)), ("bad_K+no_index", vq_code_index(K=0, index=None)),
                             ("no_index", vq_code_index(index=None)), ("no_index_of_an_empty_model", vq_code_index(N=0, index=None)),
                             ("no_slot", vq_code_index(slot=None)), ("no_scratch", vq_code_index(scratch=None))])
    add("lg_vq_ema_step", [("n_0", vq_ema_step(n=0)), ("n_2^30", vq_ema_step(n=1 << 30)), ("K_0", vq_ema_step(K=0)), ("d_0", vq_ema_step(d=0)), ("d_64", vq_ema_step(d=64)),
                           ("bad_d+no_x", vq_ema_step(d=64, x=None)), ("no_x", vq_ema_step(x=None)), ("no_embed", vq_ema_step(embed=None)),
                           ("no_cluster_size", vq_ema_step(size=None)), ("no_out_index", vq_ema_step(out=None)), ("no_scratch", vq_ema_step(scratch=None))])
    add("lg_compact_rows", [("negative_N", compact_rows(N=-1)), ("negative_num_tensors", compact_rows(n=-1)), ("33_tensors", compact_rows(tensors=((P, P, 12),) * 33)),
                            ("bad_count+no_dest", compact_rows(n=-1, dest=None)), ("no_dest", compact_rows(dest=None)), ("no_tables", compact_rows(tables=False)),
                            ("no_dest+bad_row", compact_rows(dest=None, tensors=((P, P, 0),))),
                            ("row_bytes_0", compact_rows(tensors=((P, P, 0),))), ("row_bytes_6", compact_rows(tensors=((P, P, 6),))),
                            ("null_src", compact_rows(tensors=((None, P, 12),))), ("null_dst", compact_rows(tensors=((P, None, 12),))),
                            ("misaligned_src", compact_rows(tensors=((ODD, P, 12),))), ("misaligned_dst", compact_rows(tensors=((P, ODD, 12),))),
                            ("second_tensor_bad", compact_rows(tensors=((P, P, 12), (P, P, -4))))])
    XYZ, SCALING, ZERO = _lib.DENSIFY_XYZ, _lib.DENSIFY_SCALING, _lib.DENSIFY_ZERO
    add("lg_densify_rows", [
        ("negative_N", densify_rows(N=-1)), ("N_2^30", densify_rows(N=1 << 30, N_out=0)), ("bad_N+bad_N_out", densify_rows(N=-1, N_out=-1)),
        ("negative_N_out", densify_rows(N_out=-1)), ("N_out_beyond_2N", densify_rows(N_out=21)), ("bad_N_out+bad_count", densify_rows(N_out=21, n=-1)),
        ("negative_num_tensors", densify_rows(n=-1)), ("33_tensors", densify_rows(tensors=(dict(),) * 33)), ("bad_count+bad_noise", densify_rows(n=-1, noise_rows=-1)),
        ("negative_noise_rows", densify_rows(noise_rows=-1)), ("noise_rows_without_noise", densify_rows(noise=None)),
        ("bad_noise+no_table", densify_rows(noise_rows=-1, table=False)), ("no_table", densify_rows(table=False)),
        ("no_table+no_map", densify_rows(table=False, map_=None)), ("no_map", densify_rows(map_=None)), ("no_record", densify_rows(record=None)),
        ("misaligned_map", densify_rows(map_=P4)), ("misaligned_record", densify_rows(record=ODD)), ("no_map+unknown_role", densify_rows(map_=None, tensors=(dict(role=9),))),
        ("role_negative", densify_rows(tensors=(dict(role=-1),))), ("role_5", densify_rows(tensors=(dict(role=5),))),
        ("unknown_role+row_words_0", densify_rows(tensors=(dict(role=5, words=0),))), ("row_words_0", densify_rows(tensors=(dict(words=0),))),
        ("row_words_0+null_dst", densify_rows(tensors=(dict(words=0, dst=None),))), ("null_dst", densify_rows(tensors=(dict(dst=None),))),
        ("null_src", densify_rows(tensors=(dict(src=None),))), ("null_dst_of_a_zero_role", densify_rows(tensors=(dict(role=ZERO, src=None, dst=None),))),
        ("null_dst+misaligned_src", densify_rows(tensors=(dict(dst=None, src=ODD),))), ("misaligned_src", densify_rows(tensors=(dict(src=ODD),))),
        ("misaligned_dst", densify_rows(tensors=(dict(dst=ODD),))), ("misaligned+xyz_row_words", densify_rows(tensors=(dict(dst=ODD, role=XYZ, words=4),))),
        ("xyz_row_words_4", densify_rows(tensors=(dict(role=XYZ, words=4),))), ("scaling_row_words_1", densify_rows(tensors=(dict(role=SCALING, words=1),))),
        ("xyz_row_words+no_rotation", densify_rows(tensors=(dict(role=XYZ, words=4),), rotation=None)),
        ("xyz_without_rotation", densify_rows(tensors=(dict(role=XYZ),), rotation=None)), ("xyz_without_scaling", densify_rows(tensors=(dict(role=XYZ),), scaling=None)),
        ("xyz_misaligned_rotation", densify_rows(tensors=(dict(role=XYZ),), rotation=ODD)), ("xyz_misaligned_noise", densify_rows(tensors=(dict(role=XYZ),), noise=ODD)),
        ("second_tensor_bad", densify_rows(tensors=(dict(), dict(words=-1)))),
    ])
    add("lg_filter3d_update", [("negative_N", filter3d_update(N=-1)), ("N_2^30", filter3d_update(N=1 << 30)), ("bad_N+V_0", filter3d_update(N=-1, V=0)),
                               ("V_0", filter3d_update(V=0)), ("V_0+no_means", filter3d_update(V=0, means=None)), ("no_means", filter3d_update(means=None)),
                               ("no_cameras", filter3d_update(cameras=None)), ("no_filter", filter3d_update(filt=None)), ("no_scratch", filter3d_update(scratch=None)),
                               ("no_scratch+misaligned", filter3d_update(scratch=None, means=ODD)), ("misaligned_means", filter3d_update(means=ODD)),
                               ("misaligned_cameras", filter3d_update(cameras=ODD)), ("misaligned_scratch_of_an_empty_model", filter3d_update(N=0, scratch=ODD))])
    for name, build, outs in (("lg_filter3d_apply", filter3d_apply, ("out_s", "out_o")), ("lg_filter3d_apply_bwd", filter3d_apply_bwd, ("ds", "do", "out_s", "out_o"))):
        add(name, [("negative_N", build(N=-1)), ("N_2^30", build(N=1 << 30)), ("bad_N+null", build(N=-1, scaling=None)), ("no_scaling", build(scaling=None)),
                   ("no_opacity", build(opacity=None)), ("no_filter", build(filt=None)), ("misaligned_scaling+null_later", build(scaling=ODD, **{outs[-1]: None})),
                   ("misaligned_scaling", build(scaling=ODD)), ("null_tensor_of_an_empty_model", build(N=0, filt=None))]
                  + [("no_" + o, build(**{o: None})) for o in outs] + [("misaligned_" + o, build(**{o: ODD})) for o in outs])
    return out


CASES = _cases()
IDS = [name for name, _ in CASES]
assert len(set(IDS)) == len(IDS), "two cases share an id"


def _run(call):
    fn, args = call
    lib = _lib.load()
    rc = getattr(lib, fn)(*args)
    return [rc, lib.lg_last_error().decode()]


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_and_recording_name_the_same_cases():
    golden = _golden()
    assert sorted(golden) == sorted(IDS)
    assert all(rc == _lib.LG_ERR_INVALID_ARGUMENT for rc, _msg in golden.values())      # none of them reached the HIP runtime when recorded
    covered = {name.split("/")[0] for name in IDS}
    assert covered >= {"lg_adam_step", "lg_adam_step_rows", "lg_backward", "lg_backward_chunked", "lg_backward_abs", "lg_backward_features", "lg_backward_camera",
                       "lg_blend_features", "lg_blend_features_backward", "lg_loss_forward", "lg_loss_backward", "lg_sh_grad_from_rgb", "lg_vq_colors",
                       "lg_vq_colors_bwd", "lg_vq_code_index", "lg_vq_ema_step", "lg_compact_rows", "lg_densify_rows", "lg_filter3d_update",
                       "lg_filter3d_apply", "lg_filter3d_apply_bwd"}
    for fn in covered:                                                                      # precedence: two conditions failing at once
        assert any(name.startswith(fn + "/") and "+" in name for name in IDS), fn


@pytest.mark.parametrize("fn", sorted({name.split("/")[0] for name in IDS}))
def test_refusal_code_and_message(fn):
    """Every case of one entry point; all that differ are shown."""
    golden = _golden()
    got = {name: _run(call) for name, call in CASES if name.split("/")[0] == fn}
    assert len(got) >= 9
    assert {k: v for k, v in got.items() if v != golden[k]} == {}


if __name__ == "__main__":
    table = {}
    for name, call in CASES:
        table[name] = _run(call)
        assert table[name][0] == _lib.LG_ERR_INVALID_ARGUMENT, (name, table[name])
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(table)} refusals recorded from {_lib.LIB_PATH}")
