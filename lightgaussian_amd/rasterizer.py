"""Drop-in for the `diff_gaussian_rasterization` module of the reference.

Mirrors the Python surface the reference binds to at
  gaussian_renderer/__init__.py:14-17   import GaussianRasterizationSettings, GaussianRasterizer
  gaussian_renderer/__init__.py:52-66   13-field settings record (incl. LightGaussian's f_count)
  gaussian_renderer/__init__.py:106-115 rasterizer(means3D=..., means2D=..., shs=..., colors_precomp=...,
                                                   opacities=..., scales=..., rotations=..., cov3D_precomp=...)
                                        -> (color, radii)
  gaussian_renderer/__init__.py:209-218 with f_count=True -> (gaussians_count, important_score, color, radii)
and the stale variant gaussian_renderer/gaussian_count.py:69,112 (ctor kw f_count, .forward_counter()).

All arithmetic runs in liblightgaussian_hip.so (hand-written gfx950 kernels) through the C ABI of
include/lightgaussian.h; torch supplies device memory, the current stream and autograd plumbing.
"""
import ctypes as C
import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    f_count: bool = False


# Knobs that are not part of the reference API.  _OPTIONS holds the PROCESS DEFAULTS (set_option); every forward takes a
# snapshot -- defaults, then the calling thread's `with options(...)` blocks, then the call's own `options=` argument -- and the
# snapshot travels with the call (lg_view.flags / lg_view.segment_length) and into its backward.  Library code never mutates
# the defaults: prune_list_sharded and backward_over_views pass what they need per call / per thread.
_OPTIONS = {"weight_policy": _lib.WEIGHT_OPACITY, "fast_exp": True, "profile": False, "skip_color_in_count": False,
            "fuse_getters": True, "sync_free": "validated", "max_depth": 100.0, "capacity_margin": 1.25,
            "segment_length": 0, "long_tiles": "auto", "count_long_tiles": "serial", "camera_grad": False, "antialiasing": False,
            "filter_3d": True, "absgrad": False, "score_reduce": "sum",
            # cross-check switches of the tests: never needed in production, never read from the environment
            "sh_jacobian": True, "narrow_key": False, "sort_all_bits": False, "k1_lds": False, "count_wide_band": False}
_PER_CALL_ONLY = ("pending", "tag", "status_override", "differentiated", "sh_grad_sink", "score_out", "count_sum")
_LONG_TILES = ("serial", "auto", "parallel")
_STRICT_BOOL = ("camera_grad", "antialiasing", "filter_3d", "absgrad")      # options that refuse anything but True / False
_tls = threading.local()


SCORE_REDUCTIONS = ("sum", "max")
# LG_FLAG_SCORE_MAX of the extension header include/lightgaussian_score.h (tests/test_scoremax_host.py holds the two together; the
# constants of _lib are those of lightgaussian.h)
FLAG_SCORE_MAX = 65536
WEIGHT_POLICIES = {"one": _lib.WEIGHT_ONE, "opacity": _lib.WEIGHT_OPACITY, "alpha": _lib.WEIGHT_ALPHA, "alpha_t": _lib.WEIGHT_ALPHA_T}


def weight_policy_id(value):
    """_lib.WEIGHT_* of a policy given by number or by name ("one" | "opacity" | "alpha" | "alpha_t")."""
    if isinstance(value, str):
        if value.lower() not in WEIGHT_POLICIES:
            raise ValueError(f"weight_policy must be one of {tuple(WEIGHT_POLICIES)} (or a _lib.WEIGHT_* number)")
        return WEIGHT_POLICIES[value.lower()]
    if int(value) not in WEIGHT_POLICIES.values():
        raise ValueError(f"weight_policy {value!r}: not a _lib.WEIGHT_* value")
    return int(value)


def score_reduce_name(value):
    """"sum" | "max", as given to the option score_reduce (any letter case)."""
    if not isinstance(value, str) or value.lower() not in SCORE_REDUCTIONS:
        raise ValueError(f"score_reduce must be one of {SCORE_REDUCTIONS}")
    return value.lower()


def check_score_reduce(score_reduce, weight_policy):
    """score_reduce="max" is defined for the per-hit policies only: with "one" / "opacity" every hit of a Gaussian adds the same
    value, and the maximum of equal addends is the addend -- there is nothing to compute.  Raises ValueError; returns the name."""
    name = score_reduce_name(score_reduce)
    if name == "max" and weight_policy_id(weight_policy) not in (_lib.WEIGHT_ALPHA, _lib.WEIGHT_ALPHA_T):
        raise ValueError('score_reduce="max" needs weight_policy "alpha" or "alpha_t" (every hit of "one" / "opacity" adds the same value)')
    return name


def _validate(name, value):
    if name == "weight_policy":
        weight_policy_id(value)
    if name == "score_reduce":
        score_reduce_name(value)
    if name == "long_tiles" and value not in _LONG_TILES:
        raise ValueError(f"long_tiles must be one of {_LONG_TILES}")
    if name == "count_long_tiles" and value not in ("serial", "parallel"):
        raise ValueError("count_long_tiles must be 'serial' or 'parallel'")
    if name in _STRICT_BOOL and not isinstance(value, bool):
        raise ValueError(f"{name} must be True or False")
    if name == "segment_length" and (int(value) < 0 or (int(value) != 0 and (int(value) < 64 or int(value) % 64))):
        raise ValueError("segment_length must be 0 (library default, 512) or a multiple of 64")


def _check_options(kw):
    for k, v in kw.items():
        if k not in _OPTIONS and k not in _PER_CALL_ONLY:
            raise KeyError(k)
        _validate(k, v)


def set_option(name, value):
    """Process default of one knob; returns the previous value.  (Per call: `options=` of GaussianRasterizer / render /
    count_render; per thread: `with rasterizer.options(...)`.)
    weight_policy: what one (pixel, Gaussian) hit adds to important_score -- _lib.WEIGHT_* or its name: "opacity" (default: sigma_j,
              LightGaussian's published Global Significance Score), "one" (score == hit count), "alpha" (the blending weight
              alpha_j of the hit) or "alpha_t" (alpha_j T, the hit's share of the pixel).  Every policy is deterministic and
              bit-pinned by the parity tests: the first two derive the fp32 score from the integer hit count, the per-hit ones add
              64-bit fixed-point weights (Q24.40) -- no float atomics anywhere;
    score_reduce: "sum" (default) | "max": how a count forward reduces the per-hit weights of a Gaussian over the view.  "max" (per-hit
              policies only: "alpha" / "alpha_t"; ValueError with "one" / "opacity" before any native call) makes important_score the LARGEST
              weight of any hit -- with "alpha_t" the largest share the Gaussian has of any pixel of the view, RadSplat's pruning score once
              the views are folded with a maximum (prune_list / prune_list_sharded do) -- the fp32 value the blend computed, unrounded
              (LG_FLAG_SCORE_MAX).  gaussians_count and the image are unchanged; render() ignores the option;
    fast_exp (default True): hardware exp/rcp in render() -- training renders; set False for the canonical,
              bit-pinned arithmetic.  count renders (f_count=True) ALWAYS use the canonical arithmetic;
    profile: record per-kernel hipEvent timings (read with _lib.profile_read());
    fuse_getters (default True): gaussian_renderer.render() evaluates the getters of a reference GaussianModel inside the
              kernels (LG_FLAG_RAW_PARAMS) instead of in torch; False = the reference's literal getter pattern;
    skip_color_in_count: count renders do not evaluate colours and do not write the image (the returned `render` tensor is
              uninitialised memory); for passes that only consume gaussians_count / important_score, e.g. prune_list_sharded;
    sync_free: False = every forward takes the exact path (lg_forward: the device idles while the host reads the instance
              count, allocates and launches the rest, as in the reference extension).
              "validated" (default) = lg_forward_bounded with host status: the whole view is enqueued against a capacity learnt from
              earlier views of the same shape, then the host waits for the status words that left behind K2 -- same
              guarantees as the exact path (an overflowing view is re-run at once, transparently), no idle device.
              True = nothing is read back at all, so one host thread can keep several views in flight on several streams.  The binning buffer is sized capacity_margin x the
              largest instance count seen so far for this (N, W, H) (the first view of a shape takes the exact path to learn it)
              and depths are laid out for max_depth (the camera's zfar; scene/cameras.py:64 uses 100).  A view that does not fit
              is abandoned on the device; PendingBatch.resolve() / pending_status() (one sync for a whole batch of views)
              reports it and raises the capacity, and the caller re-renders -- parallel.backward_over_views and the sharded
              prune pass do;
    segment_length: entries per backward segment of a long tile list (0 = the library default 512; tests use 64 / 128);
              travels in lg_view.segment_length, the backward of a view uses the value its forward ran with;
    long_tiles: "serial" | "auto" (default) | "parallel": walk of outlier tile lists in training forwards; "auto" is
              decided on the device from the view's own list statistics -- no dependence on earlier views;
    count_long_tiles: "serial" (default) | "parallel": the same choice for the significance-only count pass (skip_color_in_count, integer
              weights), which has a parallel long-tile walk of its own (lg_count_seg / _rewalk / _fixup; bit-identical counts).  An option of
              its own since round 6: the walk measured SLOWER than the serial one with several views in flight (1150 vs 1497 views/s on the
              heavy-tailed scene), so a process that sets long_tiles="parallel" for its training forwards must not get it for its prune pass
              as a side effect;
    sh_grad_sink (per call / per thread only): an object with .add(drgb [N,3], campos [3], sh_degree) -- the backward of a render
              with SH inputs then writes dL/d(rgb) per Gaussian (12 B) INSTEAD of the SH-coefficient gradients (12 M B), hands it
              to the sink right behind K9 on the current stream, and returns None for the coefficient gradients: the caller
              rebuilds them for all ranks' views at once (parallel.RankOneSHExchange; the data-parallel step of lightgaussian_amd.dp);
    score_out, count_sum (per call / per thread only; count forwards): score_out = a contiguous float32 [N] device tensor (e.g. a row of
              the caller's score matrix) that the forward writes important_score INTO -- the returned important_score is that tensor;
              count_sum = a contiguous int32 [N] device tensor to which the view's gaussians_count is ADDED by the kernel that writes the
              score (lg_view.count_sum; not atomic: one view at a time per accumulator).  Together they are prune_list's
              `gaussian_list += ...; imp_list += ...` bookkeeping (prune.py:144-155) without a torch launch per view (prune_list_sharded);
    camera_grad (default False): the render is also differentiated with respect to raster_settings.viewmatrix, .projmatrix and .campos
              (pose refinement): the backward makes its usual lg_backward call, then lg_backward_camera on the same scratch (one more
              gather of the gradient rows, float64 ordered sums: deterministic), and the three tensors receive [4,4], [4,4] and [3]
              gradients; the per-Gaussian gradients are bit-identical to those with the option off.  Off: nothing changes.  Not
              available for count renders (f_count), with sh_jacobian=False, or with a gradient-chunk hook / sh_grad_sink installed;
    antialiasing (default False): opacity compensation of the fixed 0.3-pixel screen-space blur (Mip-Splatting's 2D filter, the
              `antialiasing` switch of upstream 3DGS): every splat's opacity is scaled by sqrt(max(0.000025, det S / det(S + 0.3 I))) of
              its 2D covariance S, in K1, and K9 / lg_camera_bwd carry the gradient through the factor (LG_FLAG_ANTIALIAS).  Radii and
              the reference tile rectangles do not change; images, hit counts and the per-hit significance weights do; the "opacity"
              weight policy keeps the raw sigma_j.  gaussian_renderer.render / count_render / render_features switch it on for a `pipe`
              with a true `antialiasing` attribute.  Off: every kernel launched is the one launched before the option existed;
    filter_3d (default True): honour `pc.filter_3D` when the model has one (upstream Mip-Splatting's attribute, the 3D smoothing filter;
              lightgaussian_amd.filter3d): gaussian_renderer.render applies it raw -> raw in front of the fused rasterizer call
              (lg_filter3d_apply; gradients reach _scaling / _opacity through lg_filter3d_apply_bwd), the unfused path, count_render and
              render_features apply it to the activated getters.  A model without the attribute -- the reference's GaussianModel -- is
              not touched; False ignores the attribute.  Read by gaussian_renderer only: the rasterizer itself takes what it is handed;
    absgrad (default False): the backward of a render also leaves the ABSOLUTE screen-space mean gradients (AbsGS's homodirectional
              gradient, gsplat's `absgrad`): per Gaussian the sum over pixels of |dL/dmean2D| instead of the |sum| that means2D.grad
              holds, in which the signed pulls on a large splat straddling fine structure cancel.  The backward calls lg_backward_abs
              (K7's ABS variant + lg_absgrad_rows) and sets `means2D.absgrad` on the means2D tensor handed to the forward: float32 [N,3]
              in .grad's layout and NDC units, z = 0, rows of invisible Gaussians zero; OVERWRITTEN, not accumulated, by every backward
              (gsplat's convention).  Every other gradient, the image and the radii are bit-identical to those with the option off.
              Works on the activated and the raw (fused) path, with antialiasing, filter_3d, camera_grad, a gradient-chunk hook and an
              sh_grad_sink; densify.accumulate_stats(..., absgrad=True) consumes it.  Count renders have no backward and ignore it;
              features.render_features(geometry_grad=True) does not produce it (lg_backward_features has no ABS variant) and does not
              raise, so a process-wide default is safe.  Off: every kernel launched is the one launched before the option existed;
    count_wide_band: tests only -- LG_FLAG_COUNT_WIDE_BAND (the parallel long-tile count walk sends many more pixels through its exact fix-up);
    sh_jacobian / narrow_key / sort_all_bits / k1_lds: cross-check switches for the tests (K9 re-reads the SH coefficients instead
              of K1's saved direction Jacobian; the sort key laid out as if 40 bits were available; every key bit through the
              global radix passes; K1's LDS-staged SH reads).  Options like everything else (r4 verdict: they used to be read
              from os.environ on every call, where a stray variable in a user's shell would silently change the sort)."""
    if name not in _OPTIONS:
        raise KeyError(name)
    _validate(name, value)
    prev = _OPTIONS[name]
    _OPTIONS[name] = value
    return prev


class options:
    """Thread-local option overrides for everything rendered inside the `with` block on THIS host thread:

        with rasterizer.options(sync_free=True, skip_color_in_count=True):
            count_render(cam, gaussians, pipe, bg)

    Other threads keep their own view of the options; blocks nest (inner wins).  Besides the knobs of set_option: `pending`
    (a PendingBatch that collects the status words of sync-free forwards instead of the process-wide list), `tag` (recorded
    with each of them) and `status_override` (a [4] int32 tensor the next sync-free forward writes its status words to)."""

    def __init__(self, **kw):
        _check_options(kw)
        self.kw = kw

    def __enter__(self):
        _tls.stack = getattr(_tls, "stack", ()) + (self.kw,)
        return self

    def __exit__(self, *exc):
        _tls.stack = _tls.stack[:-1]
        return False


def resolve_options(overrides=None):
    """Snapshot of the options one forward runs with: process defaults < this thread's `with options(...)` blocks < overrides."""
    o = dict(_OPTIONS)
    for kw in getattr(_tls, "stack", ()):
        o.update(kw)
    if overrides:
        _check_options(overrides)
        o.update(overrides)
    return o


_GRAD_CHUNKS = {"hook": None, "chunks": 1}


def set_grad_chunk_hook(hook, chunks=4):
    """hook(first, count, grads) is called from inside every rasterizer backward, once per range of Gaussians, right after the
    K9 launch of that range is enqueued on the current stream: rows [first, first + count) of the gradient tensors in `grads`
    (dict: parameter name -> tensor) are final from that point of the stream on.  Used by parallel.OverlappedGradAllReduce to
    all-reduce finished ranges while K9 computes the next one.  hook=None restores the single-launch backward."""
    _GRAD_CHUNKS["hook"] = hook
    _GRAD_CHUNKS["chunks"] = max(1, int(chunks)) if hook is not None else 1


def _call_backward(lib, args, grads_by_name, abs_out=None):
    """lg_backward, or lg_backward_chunked when a gradient-chunk hook is installed; with abs_out (option absgrad: a float32 [N,3] tensor
    that receives the absolute mean gradients) lg_backward_abs, which takes the chunked call's arguments.  An exception raised by the hook cannot
    cross the C frame (ctypes would print and swallow it, and the remaining ranges would still be reported): it is recorded,
    the hook is not called again for this backward, and it is re-raised here once the library call has returned."""
    hook = _GRAD_CHUNKS["hook"]
    if hook is None:
        return lib.lg_backward(*args) if abs_out is None else lib.lg_backward_abs(*args, 1, _lib.CHUNK_FN(), None, _lib.ptr(abs_out))      # (a NULL callback)
    errors = []

    def _cb(_user, first, count):
        if errors:
            return
        try:
            hook(int(first), int(count), grads_by_name)
        except BaseException as e:  # noqa: BLE001 -- re-raised below, on the Python side of the call
            errors.append(e)

    cb = _lib.CHUNK_FN(_cb)
    if abs_out is None:
        rc = lib.lg_backward_chunked(*args, int(_GRAD_CHUNKS["chunks"]), cb, None)
    else:
        rc = lib.lg_backward_abs(*args, int(_GRAD_CHUNKS["chunks"]), cb, None, _lib.ptr(abs_out))
    if errors:
        raise errors[0]
    return rc


_ptr, _stream = _lib.ptr, _lib.stream       # (importable from here as before)


def _prep(t, dev):
    """contiguous fp32 tensor on dev, or None for None / empty placeholders."""
    if t is None or t.numel() == 0:
        return None
    if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
        t = t.to(device=dev, dtype=torch.float32).contiguous()
    return t


class _Call:
    """Holds the tensors referenced by the C structs alive for the duration of a call."""

    def __init__(self, rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, exact, sh_rest=None, raw=False, opts=None,
                 differentiated=False):
        opts = opts if opts is not None else resolve_options()
        self.opts = opts
        dev = means3D.device
        if dev.type != "cuda":
            raise RuntimeError("lightgaussian_amd rasterizer needs tensors on a HIP device (torch 'cuda'); there is no CPU path")
        self.dev = dev
        self.means3D = _prep(means3D, dev)
        self.sh = _prep(sh, dev)
        self.colors = _prep(colors_precomp, dev)
        self.opac = _prep(opacities, dev)
        self.scales = _prep(scales, dev)
        self.rots = _prep(rotations, dev)
        self.cov = _prep(cov3D_precomp, dev)
        self.bg = _prep(rs.bg, dev)
        self.vm = _prep(rs.viewmatrix, dev)
        self.pm = _prep(rs.projmatrix, dev)
        self.cp = _prep(rs.campos, dev)
        self.sh_rest = _prep(sh_rest, dev)
        N = self.means3D.shape[0] if self.means3D is not None else 0
        M = 0 if self.sh is None else int(self.sh.shape[1]) + (0 if sh_rest is None else int(sh_rest.shape[1]))
        flags = _lib.FLAG_RAW_PARAMS if raw else 0
        if differentiated and opts["sh_jacobian"]:     # (sh_jacobian=False, cross-check: K9 reads the SH coefficients as in rounds 1-3)
            # a backward will follow: K1 leaves the SH direction Jacobian (36 B per visible Gaussian) so that K9 need not read the
            # coefficients again (LG_FLAG_SAVE_SH_JACOBIAN).  `differentiated` is decided where grad mode is still visible
            # (_wants_grad below): no-grad forwards -- evaluation, teacher renders, the significance pass -- do not pay the write
            flags |= _lib.FLAG_SAVE_SH_JACOBIAN
        if rs.debug:
            flags |= _lib.FLAG_DEBUG
        if opts["fast_exp"] and not exact:
            flags |= _lib.FLAG_FAST_EXP
        flags |= _lib.profile_flag(opts["profile"])
        if exact and opts["skip_color_in_count"]:
            flags |= _lib.FLAG_SKIP_COLOR
        if exact and check_score_reduce(opts.get("score_reduce", "sum"), opts["weight_policy"]) == "max":      # (raises before any native call)
            flags |= FLAG_SCORE_MAX
        if exact:       # count forward: its own switch (the training forward's long_tiles does not reach the significance pass)
            flags |= _lib.FLAG_LONG_PARALLEL if opts["count_long_tiles"] == "parallel" else _lib.FLAG_LONG_SERIAL
        else:
            flags |= {"serial": _lib.FLAG_LONG_SERIAL, "auto": 0, "parallel": _lib.FLAG_LONG_PARALLEL}[opts["long_tiles"]]
        # cross-check switches (tests pass them as options)
        if opts["narrow_key"]:
            flags |= _lib.FLAG_NARROW_KEY
        if opts["sort_all_bits"]:
            flags |= _lib.FLAG_SORT_ALL_BITS
        if opts["k1_lds"]:
            flags |= _lib.FLAG_K1_LDS
        if opts["count_wide_band"]:
            flags |= _lib.FLAG_COUNT_WIDE_BAND
        if opts["antialiasing"]:    # (the backward's _Call is built from the forward's snapshot: the two cannot disagree)
            flags |= _lib.FLAG_ANTIALIAS
        if opts.get("absgrad") and not exact:   # read by lg_backward_abs alone (_backward); every forward ignores it
            flags |= _lib.FLAG_ABSGRAD
        self.view = _lib.lg_view(int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy),
                                 _lib.ptr(self.bg), float(rs.scale_modifier), _lib.ptr(self.vm), _lib.ptr(self.pm),
                                 int(rs.sh_degree), _lib.ptr(self.cp), int(bool(rs.prefiltered)), flags, int(opts["segment_length"]))
        self.g = _lib.lg_gaussians(N, M, _lib.ptr(self.means3D), _lib.ptr(self.sh), _lib.ptr(self.colors), _lib.ptr(self.opac),
                                   _lib.ptr(self.scales), _lib.ptr(self.rots), _lib.ptr(self.cov), _lib.ptr(self.sh_rest))
        self.N, self.M = N, M


def _bare_view(rs, flags, segment_length):
    """An lg_view without pointers, for the calls that read only its size, flags and segment length."""
    return _lib.lg_view(int(rs.image_height), int(rs.image_width), float(rs.tanfovx), float(rs.tanfovy), None, float(rs.scale_modifier),
                        None, None, int(rs.sh_degree), None, 0, int(flags), int(segment_length))


# ---- sync-free forwards: capacity bookkeeping --------------------------------------------------------------------------
_CAP_LOCK = threading.Lock()
_CAPACITY = {}      # (device index, N, W, H) -> binning capacity in instances


class PendingBatch:
    """Status words of sync-free forwards (option sync_free=True) that have not been looked at yet.  A caller that keeps several
    views in flight passes its own batch (`options(pending=batch, tag=k)`) and resolves it once: nothing another caller or
    thread renders meanwhile can get mixed into it.  Forwards issued without one land in the process-wide batch behind
    pending_status()."""

    def __init__(self):
        self.items = []         # (status tensor [4] int32 or None, capacity key, tag)
        self.lock = threading.Lock()

    def add(self, status, key, tag):
        with self.lock:
            self.items.append((status, key, tag))

    def __len__(self):
        return len(self.items)

    def drop_oldest(self, n):
        """Forget the n oldest entries without looking at them."""
        with self.lock:
            del self.items[:n]

    def resolve(self, capacity_margin=None):
        """[(tag, abandoned)] in issue order: abandoned = the view did not fit its binning capacity, or held a depth beyond
        max_depth, and must be re-rendered (its image is the background, its counts / scores / gradients are zero).  ONE host
        sync for the whole batch; the streams that issued the views must have been joined into the current stream.
        Capacities are raised from the instance counts the device reported (times capacity_margin: default = the option as
        resolved for the calling thread), so the re-render (and later views of that shape) fit.  An implausible count (>= 2^30:
        a status word that was never written) abandons the view but does not touch the capacity."""
        margin = float(capacity_margin if capacity_margin is not None else resolve_options()["capacity_margin"])
        with self.lock:
            pend, self.items = self.items, []
        if not pend:
            return []
        live = [p[0] for p in pend if p[0] is not None]
        it = iter(torch.stack([t.to(live[0].device) for t in live]).cpu().tolist() if live else [])
        out = []
        for st, key, tag in pend:
            if st is None:                              # this forward took the exact path (first view of its shape)
                out.append((tag, False))
                continue
            flags, _viol, _dmax, R = next(it)
            flags &= 0xFFFFFFFF
            R &= 0xFFFFFFFF
            out.append((tag, flags != 0))
            with _CAP_LOCK:
                if flags & 2:
                    _CAPACITY[key] = -1                # depth bound violated: this shape goes back to the exact path
                elif R < (1 << 30) and (flags or key in _CAPACITY) and _CAPACITY.get(key, 0) >= 0:
                    _CAPACITY[key] = max(_CAPACITY.get(key, 0), int(R * margin) + 4096)
        return out


_PENDING = PendingBatch()    # forwards issued without a batch of their own
_PENDING_CAP = 4096          # a caller that never polls must not accumulate device tensors without bound


def pending_status():
    """Outcome of every sync-free forward issued WITHOUT a PendingBatch of its own since the last call, in issue order: a list
    of booleans, True = abandoned on the device (see PendingBatch.resolve)."""
    return [bad for _tag, bad in _PENDING.resolve()]


def pending_overflow():
    """True when any sync-free forward since the last check was abandoned on the device (see pending_status)."""
    return any(pending_status())


def _note_pending(opts, status, key):
    batch = opts.get("pending")
    if batch is None:
        batch = _PENDING
        if len(batch) >= _PENDING_CAP:
            # nobody polls.  The oldest entries are dropped UNREAD: their status words may have been written on streams this
            # thread never joined (reading them here would be a blocking copy of possibly uninitialised memory in the middle of a
            # forward, and a garbage instance count would inflate the capacity of the shape)
            batch.drop_oldest(_PENDING_CAP // 2)
    batch.add(status, key, opts.get("tag"))


def _note_count(key, R, opts=None):
    with _CAP_LOCK:
        want = int(R * (opts or _OPTIONS)["capacity_margin"]) + 4096
        have = _CAPACITY.get(key, 0)
        if have >= 0 and want > have:
            _CAPACITY[key] = want


def _check_row(name, t, dtype, dev, N):
    if not (torch.is_tensor(t) and t.dtype == dtype and t.device == dev and t.shape == (N,) and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} [N] tensor on the Gaussians' device")


def _native_forward(lib, call, rs, count):
    """One forward through the C ABI.  Exact path (lg_forward / lg_forward_count: one blocking read of the instance count,
    as the reference extension) or, with option sync_free and a known capacity for this shape, lg_forward_bounded.
    Returns (color, radii, gcount, score, geom, binning, img, num_rendered)."""
    opts = call.opts
    dev, N = call.dev, call.N
    H, W = int(rs.image_height), int(rs.image_width)
    stream = _lib.stream()
    u8 = dict(dtype=torch.uint8, device=dev)
    geom = torch.empty(lib.lg_geom_bytes(N), **u8)
    img = torch.empty(lib.lg_img_bytes(W, H), **u8)
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((N,), dtype=torch.int32, device=dev)
    gcount = torch.empty((N,), dtype=torch.int32, device=dev) if count else None
    score = None
    if count:
        score = opts.get("score_out")
        if score is None:
            score = torch.empty((N,), dtype=torch.float32, device=dev)
        else:
            _check_row("score_out", score, torch.float32, dev, N)
        csum = opts.get("count_sum")
        if csum is not None:
            _check_row("count_sum", csum, torch.int32, dev, N)
            call.view.count_sum = csum.data_ptr() if N > 0 else None
    key = (dev.index, N, W, H)
    mode = opts["sync_free"]
    S = int(opts["segment_length"])
    cap = _CAPACITY.get(key) if (mode and N > 0 and not rs.prefiltered) else None
    if cap is not None and cap > 0:          # (-1: a depth beyond max_depth was seen for this shape -> exact path for good)
        binning = torch.empty(lib.lg_binning_bytes(cap, W, H, S), **u8)
        # "validated": everything of the view is enqueued, then the host waits for the four status words that left right behind
        # K2: it knows R and the abort flags before returning (safe drop-in), the device never idled.  Otherwise the words go to a
        # device tensor nobody waits for (status_override: a caller-owned [4] int32 tensor that receives them)
        host = status = None
        if mode == "validated":
            host = (C.c_uint32 * 4)()
        else:
            status = opts.get("status_override")
            if status is None:
                status = torch.empty(4, dtype=torch.int32, device=dev)
        rc = lib.lg_forward_bounded(C.byref(call.view), C.byref(call.g), _lib.ptr(geom), _lib.ptr(img), _lib.ptr(binning), cap,
                                    float(opts["max_depth"]), weight_policy_id(opts["weight_policy"]), _lib.ptr(color), _lib.ptr(radii),
                                    _lib.ptr(gcount), _lib.ptr(score), _lib.ptr(status), None if host is None else C.byref(host), stream)
        _lib.check(rc)
        if host is None:
            _note_pending(opts, status, key)
            return color, radii, gcount, score, geom, binning, img, cap
        if host[0] == 0:
            _note_count(key, int(host[3]), opts)
            return color, radii, gcount, score, geom, binning, img, cap
        with _CAP_LOCK:                        # the view did not fit (its kernels were no-ops): exact path below, same buffers
            if host[0] & 2:
                _CAPACITY[key] = -1
            else:
                _CAPACITY[key] = int(int(host[3]) * opts["capacity_margin"]) + 4096
        del binning
    holder = {}

    def _alloc(_user, nbytes):
        holder["t"] = _lib.scratch(nbytes, dev)
        return holder["t"].data_ptr()

    cb = _lib.ALLOC_FN(_alloc)
    bin_ptr = C.c_void_p()
    R = C.c_int64(0)
    if count:
        rc = lib.lg_forward_count(C.byref(call.view), C.byref(call.g), _lib.ptr(geom), _lib.ptr(img), cb, None,
                                  weight_policy_id(opts["weight_policy"]), _lib.ptr(color), _lib.ptr(radii), _lib.ptr(gcount), _lib.ptr(score),
                                  C.byref(bin_ptr), C.byref(R), stream)
    else:
        rc = lib.lg_forward(C.byref(call.view), C.byref(call.g), _lib.ptr(geom), _lib.ptr(img), cb, None, _lib.ptr(color), _lib.ptr(radii),
                            C.byref(bin_ptr), C.byref(R), stream)
    _lib.check(rc)
    if mode:
        _note_count(key, int(R.value), opts)
        if mode != "validated":
            _note_pending(opts, None, key)         # keeps the batch aligned with the issue order
    return color, radii, gcount, score, geom, holder.get("t"), img, int(R.value)


def _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp):
    # same messages/semantics as the published rasterizer's forward()
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception("Please provide excatly one of either SHs or precomputed colors!")
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
       ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")


class _GradSet:
    """The per-Gaussian gradient buffers of one backward, by slot.  SLOTS is the order in which lg_backward, lg_backward_chunked
    and lg_backward_features take their nine dL_d* pointers (include/lightgaussian.h); a slot whose input the call does not have
    is None.  rgb_only: SH inputs whose backward writes dL/d(rgb) to the `colors` slot INSTEAD of the coefficient gradients (an
    sh_grad_sink).  new: torch.empty, or torch.zeros where no kernel is going to write the buffers."""
    SLOTS = ("means2D", "means3D", "shs", "colors", "opacity", "scales", "rotations", "cov3D", "shs_rest")
    # what the gradient-chunk hook calls them: the rasterizer's argument names, and GaussianModel's parameters on the fused path
    HOOK_NAMES = {False: (("means3D", "means3D"), ("shs", "shs"), ("colors_precomp", "colors"), ("opacities", "opacity"),
                          ("scales", "scales"), ("rotations", "rotations"), ("cov3D_precomp", "cov3D")),
                  True: (("_xyz", "means3D"), ("_features_dc", "shs"), ("_features_rest", "shs_rest"), ("_opacity", "opacity"),
                         ("_scaling", "scales"), ("_rotation", "rotations"))}

    def __init__(self, call, rgb_only=False, new=None):
        f32 = dict(dtype=torch.float32, device=call.dev)
        if new is None:             # looked up per call, not bound at import: tests/poison_common.py replaces torch.empty
            new = torch.empty

        def rows(have, width):
            return new((call.N, width), **f32) if have else None

        def coeffs(t):      # ([N, M, 3]; on the fused path `shs` is _features_dc [N, 1, 3] and `shs_rest` the other rows)
            return None if (t is None or rgb_only) else new((call.N, t.shape[1], 3), **f32)

        self.rgb_only = rgb_only
        self.by_slot = {"means2D": rows(True, 3), "means3D": rows(True, 3), "shs": coeffs(call.sh),
                        "colors": rows(call.colors is not None or rgb_only, 3), "opacity": rows(True, 1),
                        "scales": rows(call.scales is not None, 3), "rotations": rows(call.rots is not None, 4),
                        "cov3D": rows(call.cov is not None, 6), "shs_rest": coeffs(call.sh_rest)}

    def __getitem__(self, slot):
        return self.by_slot[slot]

    def ptrs(self):
        return [_lib.ptr(self.by_slot[s]) for s in self.SLOTS]

    def by_hook_name(self, raw):
        """name -> tensor, as the gradient-chunk hook receives them (dL/d(rgb) of an rgb_only backward is not a parameter's)."""
        return {name: self.by_slot[s] for name, s in self.HOOK_NAMES[raw]
                if self.by_slot[s] is not None and not (self.rgb_only and s == "colors")}


def _finish_forward(ctx, rs, num_rendered, opts, means2D=None):
    """What a differentiated forward leaves on ctx for its backward, besides the saved tensors."""
    ctx.raster_settings = rs
    # option absgrad: the tensor whose .absgrad the backward sets (a plain reference: the caller's own means2D, not a saved copy)
    ctx.absgrad_target = means2D if (opts.get("absgrad") and not rs.f_count and torch.is_tensor(means2D)) else None
    ctx.num_rendered = num_rendered
    ctx.opts = {k: v for k, v in opts.items() if k not in _PER_CALL_ONLY}   # the backward runs with the forward's options
    ctx.sh_sink = opts.get("sh_grad_sink")
    # no zero tensors for outputs nobody differentiated: autograd would hand the backward a materialised int32 [N] zero for
    # `radii` on every step (12 MB fill at 3M Gaussians, measured 5.9 us per step); the backward accepts None
    ctx.set_materialize_grads(False)


def _backward(ctx, call, grad_color, radii, geom, binning, img, raw):
    """The backward of one render: lg_backward (or _chunked; lg_backward_abs with option absgrad, which also sets means2D.absgrad), then
    lg_backward_camera on its scratch (option camera_grad), then the sink.  Returns the _GradSet."""
    lib = _lib.load()
    rs, dev = ctx.raster_settings, call.dev
    if grad_color is None:
        grad_color = torch.zeros((3, int(rs.image_height), int(rs.image_width)), dtype=torch.float32, device=dev)
    grad_color = _prep(grad_color, dev)
    with torch.cuda.device(dev):
        stream = _lib.stream()
        sink = ctx.sh_sink if call.sh is not None else None
        g = _GradSet(call, rgb_only=sink is not None)
        scratch = _lib.scratch(lib.lg_backward_scratch_bytes(call.N, ctx.num_rendered), dev)
        target = getattr(ctx, "absgrad_target", None)
        # (an empty model: torch hands out NULL for empty tensors, which lg_backward_abs refuses -- the plain call, and an empty .absgrad)
        abs_out = None if (target is None or call.N == 0) else torch.empty((call.N, 3), dtype=torch.float32, device=dev)
        rc = _call_backward(lib, (C.byref(call.view), C.byref(call.g), _lib.ptr(radii), _lib.ptr(geom), _lib.ptr(binning), _lib.ptr(img),
                                  C.c_int64(ctx.num_rendered), _lib.ptr(grad_color), *g.ptrs(), _lib.ptr(scratch), stream), g.by_hook_name(raw), abs_out)
        _lib.check(rc)
        if target is not None:
            # overwritten by every backward, never accumulated
            target.absgrad = abs_out if abs_out is not None else torch.zeros((0, 3), dtype=torch.float32, device=dev)
        if ctx.opts["camera_grad"]:
            ctx.cam_grads = _camera_backward(lib, call.view, call.g, dev, radii, geom, binning, ctx.num_rendered, scratch, stream)
        if sink is not None:        # g["colors"] holds dL/d(rgb of the SH expansion); the coefficient gradients are the sink's business
            sink.add(g["colors"], call.cp, int(rs.sh_degree))
            g.by_slot["colors"] = None
    return g


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings, options=None):
        lib = _lib.load()
        rs = raster_settings
        count = bool(rs.f_count)
        opts = resolve_options(options)
        call = _Call(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, exact=count, opts=opts,
                     differentiated=opts.get("differentiated", any(ctx.needs_input_grad)))
        with torch.cuda.device(call.dev):
            color, radii, gcount, score, geom, binning, img, num_rendered = _native_forward(lib, call, rs, count)
        _finish_forward(ctx, rs, num_rendered, opts, means2D)
        ctx.save_for_backward(call.means3D, call.sh, call.colors, call.opac, call.scales, call.rots, call.cov, radii,
                              geom, binning, img)
        ctx.mark_non_differentiable(radii)
        if count:
            ctx.mark_non_differentiable(gcount, score)
            return gcount, score, color, radii
        return color, radii

    @staticmethod
    def backward(ctx, *grads):
        rs = ctx.raster_settings
        means3D, sh, colors, opac, scales, rots, cov, radii, geom, binning, img = ctx.saved_tensors
        call = _Call(rs, means3D, sh, colors, opac, scales, rots, cov, exact=bool(rs.f_count), opts=ctx.opts, differentiated=True)
        g = _backward(ctx, call, grads[2] if rs.f_count else grads[0], radii, geom, binning, img, raw=False)
        return (g["means3D"], g["means2D"], g["shs"], g["colors"], g["opacity"], g["scales"], g["rotations"], g["cov3D"], None, None)


class _RasterizeGaussiansRaw(torch.autograd.Function):
    """SURVEY 8f row 1 ("fused getters"): rasterise straight from GaussianModel's RAW parameters.  The
    activations of scene/gaussian_model.py:98-118 (exp / normalize / sigmoid) and the cat of
    _features_dc/_features_rest run inside K1, their backward inside K9 (LG_FLAG_RAW_PARAMS)."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity_logit, log_scales, raw_rotations, raster_settings, options=None):
        lib = _lib.load()
        rs = raster_settings
        opts = resolve_options(options)
        if rs.f_count:
            raise Exception("raw-parameter rasterisation is a training path; use count_render for significance")
        rest = features_rest if (features_rest is not None and features_rest.shape[1] > 0) else None
        call = _Call(rs, xyz, features_dc, None, opacity_logit, log_scales, raw_rotations, None, exact=False, sh_rest=rest, raw=True, opts=opts,
                     differentiated=opts.get("differentiated", any(ctx.needs_input_grad)))
        with torch.cuda.device(call.dev):
            color, radii, _gc, _sc, geom, binning, img, num_rendered = _native_forward(lib, call, rs, False)
        _finish_forward(ctx, rs, num_rendered, opts, means2D)
        ctx.rest_shape = None if features_rest is None else tuple(features_rest.shape)
        ctx.save_for_backward(call.means3D, call.sh, call.sh_rest, call.opac, call.scales, call.rots, radii, geom, binning, img)
        # visibility_filter (= radii > 0, gaussian_renderer/__init__.py:121) read in place: K1 leaves it as bytes in the geom buffer
        # READ-ONLY view into `geom`, which is also saved for the backward: it keeps that buffer (~70 B per Gaussian) alive for as long
        # as the caller holds visibility_filter (the trainers drop it at the end of the iteration), and an in-place write to it makes
        # autograd refuse the backward ("modified by an inplace operation") -- loud, not silent.  A clone would be one more launch
        # (~5 us) in a step whose launch gaps are already 7 % of it; callers that keep the mask use .clone() (lightgaussian_amd.dp does).
        off = lib.lg_geom_visible_offset(call.N)
        visible = geom[off:off + call.N].view(torch.bool)
        ctx.mark_non_differentiable(radii, visible)
        return color, radii, visible

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, _grad_visible=None):
        xyz, dc, rest, opac, scales, rots, radii, geom, binning, img = ctx.saved_tensors
        call = _Call(ctx.raster_settings, xyz, dc, None, opac, scales, rots, None, exact=False, sh_rest=rest, raw=True, opts=ctx.opts,
                     differentiated=True)
        g = _backward(ctx, call, grad_color, radii, geom, binning, img, raw=True)
        g_rest = g["shs_rest"]
        if g_rest is None and ctx.rest_shape is not None and not g.rgb_only:    # a model without rest rows: its empty parameter's zero
            g_rest = torch.zeros(ctx.rest_shape, dtype=torch.float32, device=call.dev)
        return g["means3D"], g["means2D"], g["shs"], g_rest, g["opacity"], g["scales"], g["rotations"], None, None


def _camera_backward(lib, view, g, dev, radii, geom, binning, num_rendered, scratch, stream):
    """lg_backward_camera right behind the lg_backward call that filled `scratch`, on the same stream: (dL/dviewmatrix [4,4],
    dL/dprojmatrix [4,4], dL/dcampos [3]) on the Gaussians' device."""
    f32 = dict(dtype=torch.float32, device=dev)
    g_vm, g_pm, g_cp = torch.empty((4, 4), **f32), torch.empty((4, 4), **f32), torch.empty((3,), **f32)
    cam_scratch = _lib.scratch(lib.lg_camera_scratch_bytes(g.N), dev)
    rc = lib.lg_backward_camera(C.byref(view), C.byref(g), _lib.ptr(radii), _lib.ptr(geom), _lib.ptr(binning), C.c_int64(num_rendered),
                                _lib.ptr(scratch), _lib.ptr(g_vm), _lib.ptr(g_pm), _lib.ptr(g_cp), _lib.ptr(cam_scratch), stream)
    _lib.check(rc)
    return g_vm, g_pm, g_cp


def _camera_empty_backward(ctx):
    """The camera gradients of an empty model (the plain backward has nothing to save and nothing to do there): lg_backward_camera
    with N = 0 writes the zeros."""
    rs, dev = ctx.raster_settings, ctx.cam_empty
    view = _bare_view(rs, 0, ctx.opts["segment_length"])
    g = _lib.lg_gaussians(0, 0, None, None, None, None, None, None, None, None)
    with torch.cuda.device(dev):
        return _camera_backward(_lib.load(), view, g, dev, None, None, None, 0, None, _lib.stream())


def _with_camera_inputs(base, doc):
    """`base` whose inputs also include the camera (option camera_grad): raster_settings.viewmatrix, .projmatrix and .campos in
    front of the usual ones.  The backward is the base class's -- which, with the option on, calls lg_backward_camera on the
    scratch of its lg_backward call -- with the three camera gradients in front."""

    def forward(ctx, viewmatrix, projmatrix, campos, *args):
        # (the kernels read the camera through raster_settings, which holds these same tensors: they are inputs here for autograd's sake)
        ctx.cam_like = tuple((t.device, t.dtype, tuple(t.shape)) for t in (viewmatrix, projmatrix, campos))
        ctx.cam_empty = args[0].device if args[0].shape[0] == 0 else None      # an empty model: see _camera_empty_backward
        ctx.cam_base_inputs = len(args)
        return base.forward(ctx, *args)

    def backward(ctx, *grads):
        if ctx.cam_empty is not None:
            ctx.cam_grads, out = _camera_empty_backward(ctx), (None,) * ctx.cam_base_inputs
        else:
            out = tuple(base.backward(ctx, *grads))
        return tuple(g.to(device=dev, dtype=dt).reshape(shape) for g, (dev, dt, shape) in zip(ctx.cam_grads, ctx.cam_like)) + out

    return type(base)(base.__name__ + "Camera", (base,), {"__doc__": doc, "__module__": __name__, "forward": staticmethod(forward),
                                                            "backward": staticmethod(backward)})


_RasterizeGaussiansCamera = _with_camera_inputs(_RasterizeGaussians, "_RasterizeGaussians with the camera among its inputs (see _with_camera_inputs).")
_RasterizeGaussiansRawCamera = _with_camera_inputs(_RasterizeGaussiansRaw, "The camera_grad twin of _RasterizeGaussiansRaw (see _with_camera_inputs).")


def option_value(name, overrides=None):
    """One knob as resolve_options(overrides)[name] would give it, without building the snapshot (a few dictionary look-ups: this
    sits in front of every render)."""
    if overrides and name in overrides:
        _validate(name, overrides[name])
        return overrides[name]
    for kw in reversed(getattr(_tls, "stack", ())):
        if name in kw:
            return kw[name]
    return _OPTIONS[name]


def _camera_grad_requested(options, rs):
    """True when the resolved options ask for camera gradients; raises where the option cannot be honoured (before any device call)."""
    if not option_value("camera_grad", options):
        return False
    opts = resolve_options(options)
    if rs.f_count:
        raise ValueError("camera_grad is not available for count renders (f_count=True)")
    if not opts["sh_jacobian"]:
        raise ValueError("camera_grad needs sh_jacobian=True: the camera centre enters through the saved SH direction Jacobian")
    if _GRAD_CHUNKS["hook"] is not None:
        raise ValueError("camera_grad is not available with a gradient-chunk hook installed (set_grad_chunk_hook)")
    if opts.get("sh_grad_sink") is not None:
        raise ValueError("camera_grad is not available with an sh_grad_sink (data-parallel steps)")
    for name in ("viewmatrix", "projmatrix", "campos"):
        if not torch.is_tensor(getattr(rs, name)):
            raise TypeError(f"camera_grad: raster_settings.{name} must be a torch tensor")
    return True


def _wants_grad(options, *tensors):
    """options + {"differentiated": will a backward follow this forward?}.  Decided HERE, outside Function.forward, where grad mode
    is still what the caller set: inside forward() autograd has already switched it off, and ctx.needs_input_grad mirrors the
    inputs' requires_grad even under torch.no_grad() -- every evaluation / teacher / significance render would set
    LG_FLAG_SAVE_SH_JACOBIAN and write 36 B per visible Gaussian for nothing."""
    want = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
    return dict(options or {}, differentiated=want)


def _rasterize(function, camera_function, inputs, rs, options):
    """function.apply on the per-Gaussian inputs of one render, or with option camera_grad camera_function.apply."""
    if _camera_grad_requested(options, rs):
        camera = (rs.viewmatrix, rs.projmatrix, rs.campos)
        return camera_function.apply(*camera, *inputs, rs, _wants_grad(options, *inputs, *camera))
    return function.apply(*inputs, rs, _wants_grad(options, *inputs))


def rasterize_gaussians_raw(xyz, means2D, features_dc, features_rest, opacity_logit, log_scales, raw_rotations, raster_settings,
                            options=None):
    return _rasterize(_RasterizeGaussiansRaw, _RasterizeGaussiansRawCamera, (xyz, means2D, features_dc, features_rest, opacity_logit, log_scales, raw_rotations), raster_settings, options)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, options=None):
    return _rasterize(_RasterizeGaussians, _RasterizeGaussiansCamera, (means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                                                        cov3Ds_precomp), raster_settings, options)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings, f_count=None, options=None):
        """raster_settings: the reference's 13-field record.  options (extension, not in the reference): a dict of per-call
        overrides of the knobs documented at set_option -- e.g. {"skip_color_in_count": True, "sync_free": True}."""
        super().__init__()
        if f_count is not None:  # stale ctor form, gaussian_renderer/gaussian_count.py:69
            raster_settings = raster_settings._replace(f_count=bool(f_count))
        self.raster_settings = raster_settings
        self.options = dict(options) if options else None

    def markVisible(self, positions):
        """Frustum test only (never called by the reference; kept for API completeness)."""
        with torch.no_grad():
            rs = self.raster_settings
            ph = torch.cat([positions, torch.ones_like(positions[:, :1])], dim=1)
            return (ph @ rs.viewmatrix.to(positions.device))[:, 2] > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, self.options)

    def forward_counter(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                        cov3D_precomp=None):
        """Stale count entry point (gaussian_renderer/gaussian_count.py:112)."""
        _check_inputs(shs, colors_precomp, scales, rotations, cov3D_precomp)
        rs = self.raster_settings._replace(f_count=True)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, rs, self.options)
