"""Python handle over the C ABI.  numpy arrays => DLM_MEM_HOST (the engine stages them),
torch CUDA tensors => DLM_MEM_DEVICE (zero-copy; PyTorch is only the allocator here)."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Union

import numpy as np

from . import _lib
from .dlm import DlmParameters, MaterialisedModel


class EngineError(RuntimeError):
    pass


def _cm(a):
    a = np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a.T).reshape(-1) if a.ndim == 2 else np.ascontiguousarray(a).reshape(-1)


def _cm_stream(a):
    """One matrix, or a [T] stream of matrices -> flat column-major array(s)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 3:
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1))).reshape(-1)
    return _cm(a)


def pack_params(params: Union[DlmParameters, Sequence[DlmParameters]], N: int):
    """DlmParameters (shared) or a sequence of N DlmParameters (per series) -> flat column-major arrays and strides
    in doubles: (V, v_stride, W, w_stride, m0, m0_stride, C0, c0_stride, v_tstride, w_tstride).  The last two are
    the per-time strides of V_t / W_t streams (0 = time-invariant)."""
    plist = [params] if isinstance(params, DlmParameters) else list(params)
    if not isinstance(params, DlmParameters) and len(plist) != N:
        raise ValueError(f"need {N} DlmParameters, got {len(plist)}")
    p0 = plist[0]
    vts = p0.v.shape[-1] ** 2 if p0.v.ndim == 3 else 0
    wts = p0.w.shape[-1] ** 2 if p0.w.ndim == 3 else 0
    if any((q.v.ndim == 3) != (vts != 0) or (q.w.ndim == 3) != (wts != 0) for q in plist):
        raise ValueError("either every series has time-varying V (W) or none")
    if isinstance(params, DlmParameters):
        return (_cm_stream(p0.v), 0, _cm_stream(p0.w), 0, _cm(p0.m0), 0, _cm(p0.c0), 0, vts, wts)
    V = np.stack([_cm_stream(q.v) for q in plist]); W = np.stack([_cm_stream(q.w) for q in plist])
    m0 = np.stack([_cm(q.m0) for q in plist]); C0 = np.stack([_cm(q.c0) for q in plist])
    return (V.reshape(-1), V.shape[1], W.reshape(-1), W.shape[1], m0.reshape(-1), m0.shape[1],
            C0.reshape(-1), C0.shape[1], vts, wts)


def _out_or_empty(be, out, name, shape, dtype=np.float64):
    """The caller's buffer out[name], or a fresh one."""
    return out[name] if out and name in out else be.empty(shape, dtype)


# where each symbol takes a data pointer (void*), counted after the handle: the arguments Engine._call turns into addresses
_POINTERS = {name: tuple(i for i, t in enumerate(args[1:]) if t is ctypes.c_void_p) for name, _, args in _lib.SYMBOLS}


def _options(be, flags=0, seed=0, series_offset=0):
    return _lib.Options(flags, be.mem, seed, series_offset)


def _outputs(be, N, status=None, **spec):
    """The outputs of a call in the order the call and the returned dict have them: every name=(wanted, shape[, dtype]) as a fresh
    buffer or None, any other value (the caller's buffer, or None) as it is, and last "status" [N] (a fresh one unless given)."""
    out = {name: (be.empty(*v[1:]) if v[0] else None) if isinstance(v, tuple) else v for name, v in spec.items()}
    out["status"] = be.empty((N,), np.int32) if status is None else status
    return out


def _model_desc(be, mat, N, *, F=None, f_stride=0, G=None, n_g=0, g_index=None, dt=None):
    """A ModelDesc of mat's shape that points at the given tables only (the others NULL) -> (descriptor, the arrays it points into:
    what the call has to keep alive)."""
    bufs = (be.put(F), be.put(G), be.put(g_index, np.int32), be.put(dt))
    Fp, Gp, gip, dtp = (None if b is None else be.ptr(b).value for b in bufs)
    return _lib.ModelDesc(mat.d, mat.p, mat.T, N, Fp, f_stride, Gp, n_g, gip, dtp), bufs


def _strided(a, k, scalar=False):
    """[k] shared by the series or [N][k], a NumPy array or a device tensor (with scalar=True also one number for all k) -> (the array,
    its stride in doubles: 0 = shared)."""
    a = a if hasattr(a, "data_ptr") else np.asarray(a, dtype=np.float64)
    if scalar and np.ndim(a) == 0:
        a = np.full(k, float(a))
    return a, k if a.ndim == 2 else 0


def check_shrinkage(a, error=None):
    """The shrinkage of the Liu-West family, 0 < a <= 1 (NaN refused); raises `error` (default: EngineError)."""
    if not 0.0 < float(a) <= 1.0:
        raise (error or EngineError)(f"the shrinkage a must satisfy 0 < a <= 1, got {a!r}")


def _counter(be, accepted, shape):
    """The caller's int32 acceptance counter (incremented in place), or a fresh one of zeros."""
    acc = be.put(np.zeros(shape, np.int32) if accepted is None else accepted, np.int32)
    if tuple(acc.shape) != tuple(shape):
        raise EngineError(f"accepted must have the shape {tuple(shape)}, got {tuple(acc.shape)}")
    return acc


def _as_prior(cls, prior):
    """A prior struct of _lib as it is, or made from its fields in order (integers where the struct has them)."""
    if isinstance(prior, cls):
        return prior
    return cls(*((float if t is ctypes.c_double else int)(x) for (_, t), x in zip(cls._fields_, tuple(prior), strict=True)))


def check_pf_shape(d: int, p: int, n_particles: int):
    """What dlm_pf_batch asks of its shape, said before anything is staged (the engine answers the same with DLM_ERR_UNSUPPORTED)."""
    if p != 1:
        raise EngineError(f"the particle filter takes a univariate observation (p = 1: every Dglm family reads y(0) and V(0,0)), got p = {p}")
    if not 1 <= d <= _lib.PF_MAX_D:
        raise EngineError(f"the particle filter takes a state of dimension 1 <= d <= {_lib.PF_MAX_D}, got d = {d}")
    if n_particles % 64 != 0 or not _lib.PF_MIN_PARTICLES <= n_particles <= _lib.PF_MAX_PARTICLES:
        raise EngineError(f"the number of particles must be a multiple of 64 between {_lib.PF_MIN_PARTICLES} and {_lib.PF_MAX_PARTICLES} "
                          f"(one wavefront per series, whole slots of particles), got {n_particles}")


def check_pf_resample(resample, mh_steps):
    """What dlm_pf_resampled asks of its resampling descriptor -> (scheme, mh_steps) as ints (the engine answers the same with
    DLM_ERR_ARG)."""
    if isinstance(resample, bool) or not isinstance(resample, (int, np.integer)) or not _lib.RESAMPLE_MULTINOMIAL <= resample <= _lib.RESAMPLE_METROPOLIS:
        raise EngineError(f"resample must be one of _lib.RESAMPLE_* (0..3), got {resample!r}")
    if isinstance(mh_steps, bool) or not isinstance(mh_steps, (int, np.integer)):
        raise EngineError(f"mh_steps must be an integer, got {mh_steps!r}")
    if resample == _lib.RESAMPLE_METROPOLIS:
        if not 1 <= mh_steps <= _lib.PF_MAX_MH_STEPS:
            raise EngineError(f"Metropolis resampling takes 1 <= mh_steps <= {_lib.PF_MAX_MH_STEPS}, got {mh_steps}")
    elif mh_steps != 0:
        raise EngineError(f"mh_steps belongs to RESAMPLE_METROPOLIS alone: it must be 0 under every other scheme, got {mh_steps}")
    return int(resample), int(mh_steps)


def check_pf_ranks(ranks, n_particles: int):
    """The order statistics dlm_pf_forecast_particles writes per time: at most PF_FORECAST_MAX_RANKS ranks, each in [0, n_particles) -> the ranks as
    a list of ints (the engine answers the same with DLM_ERR_ARG)."""
    rk = [int(r) for r in ranks]
    if len(rk) > _lib.PF_FORECAST_MAX_RANKS:
        raise EngineError(f"a forecast takes at most {_lib.PF_FORECAST_MAX_RANKS} ranks (order statistics per time), got {len(rk)}")
    if any(not 0 <= r < n_particles for r in rk):
        raise EngineError(f"a rank must satisfy 0 <= rank < n_particles = {n_particles}, got {rk}")
    return rk


def check_rb_lds(d: int, n_particles: int):
    """What dlm_rb_batch asks of (d, P) beyond check_pf_shape: every particle's covariance lives in LDS."""
    need = _lib.rb_lds_bytes(d, n_particles)
    if need > _lib.RB_LDS_BYTES:
        raise EngineError(f"the Rao-Blackwellised filter keeps every particle's covariance in LDS: d = {d} with {n_particles} particles needs "
                          f"{need} bytes of the {_lib.RB_LDS_BYTES} a workgroup gets (d <= 3: 1024 particles, d = 4: 896, d = 5: 640, "
                          "d = 6: 512, d = 7: 384, d = 8: 320, d = 9: 256, d = 10: 192, d = 11 and 12: 128, d = 13 .. 16: 64)")


def check_pf_forecast_learned_lds(d: int, n_particles: int):
    """What dlm_pf_forecast_learned asks of (d, P) beyond check_pf_shape: every particle's state variances live in LDS beside the cloud."""
    need = _lib.pf_forecast_learned_lds_bytes(d, n_particles)
    if need > _lib.RB_LDS_BYTES:
        raise EngineError(f"the forecast from a learning filter's cloud keeps every particle's variances in LDS: d = {d} with {n_particles} "
                          f"particles needs {need} bytes of the {_lib.RB_LDS_BYTES} a workgroup gets ((2 d + 3.5) n_particles doubles: "
                          "d = 16 with at most 512 particles, d <= 8 with 1024)")


def check_sv_paths_shape(k: int, horizon: int, n_paths: int):
    """What dlm_sv_paths takes: 1 <= k <= 8 chains, a horizon inside the Philox slot field, whole wavefronts of paths up to 1024."""
    if not 1 <= k <= 8:
        raise EngineError(f"k = {k}: the volatility paths take 1 <= k <= 8 factors")
    if not 1 <= horizon <= _lib.SVPATH_MAX_H:
        raise EngineError(f"horizon must satisfy 1 <= horizon <= {_lib.SVPATH_MAX_H}, got {horizon}")
    if n_paths < 64 or n_paths > _lib.SVPATH_MAX_R or n_paths % 64:
        raise EngineError(f"n_paths must be a multiple of 64 with 64 <= n_paths <= {_lib.SVPATH_MAX_R}, got {n_paths}")


def check_mixture_shape(N: int, C: int, H: int, p: int, probs):
    """What dlm_gaussian_mixture_summary takes; returns probs as a list of floats."""
    if min(N, C, H, p) < 1:
        raise EngineError(f"N, C, H, p must be >= 1, got {(N, C, H, p)}")
    if C > _lib.MIX_MAX_C:
        raise EngineError(f"C = {C}: the mixture summary takes at most 2^30 components per row")
    if p > _lib.MIX_MAX_P:
        raise EngineError(f"p = {p}: the mixture summary takes p <= {_lib.MIX_MAX_P}")
    pr = [float(q) for q in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if len(pr) > _lib.MIX_MAX_NQ:
        raise EngineError(f"at most {_lib.MIX_MAX_NQ} quantiles per call, got {len(pr)}")
    if not all(0.0 < q < 1.0 for q in pr):
        raise EngineError(f"every prob must lie inside (0, 1), got {pr}")
    return pr


def _pf_shape(mat, n_particles, family):
    """(d, T, P) of a call of one of the three particle filters, after the checks of its shape and of its family."""
    P = int(n_particles)
    check_pf_shape(mat.d, mat.p, P)
    if family not in range(6):
        raise EngineError(f"family must be one of _lib.OBS_* (0..5), got {family!r}")
    return mat.d, mat.T, P


def _pf_data(be, y, T, family, obs_param):
    """(N, y [N][T], obs_param [N] or None) of a particle-filter call on the backend; a scalar obs_param is every series'."""
    N = int(y.shape[0])
    if tuple(y.shape) not in ((N, T), (N, T, 1)):
        raise EngineError(f"y must be [N][T] = {(N, T)}, got {tuple(y.shape)}")
    yb = be.put(y).reshape(N, T)
    if family == _lib.OBS_STUDENTT and obs_param is None:
        raise EngineError("OBS_STUDENTT needs obs_param: the degrees of freedom (a scalar or one per series)")
    ob = None
    if obs_param is not None:
        ob = be.put(np.full(N, float(obs_param)) if np.ndim(obs_param) == 0 else obs_param)
        if tuple(ob.shape) != (N,):
            raise EngineError(f"obs_param must be a scalar or [N] = {(N,)}, got {tuple(ob.shape)}")
    return N, yb, ob


def _pf_priors(be, prior_w, prior_v, learn_v, N, d):
    """The priors of a learning filter on the backend with their strides in doubles (0: shared by the series):
    (prior_v or None, its stride, prior_w, its stride), the order the calls take them in."""
    pw = np.ascontiguousarray(prior_w, dtype=np.float64)
    if pw.shape not in ((d, 2), (N, d, 2)):
        raise EngineError(f"prior_w must be [d][2] = {(d, 2)} or [N][d][2], got {pw.shape}")
    pv = None
    if learn_v:
        pv = np.ascontiguousarray(prior_v, dtype=np.float64)
        if pv.shape not in ((2,), (N, 2)):
            raise EngineError(f"prior_v must be [2] or [N][2], got {pv.shape}")
    return be.put(pv), 2 if learn_v and pv.ndim == 2 else 0, be.put(pw), 2 * d if pw.ndim == 3 else 0


class _Host:
    mem = _lib.DLM_MEM_HOST

    @staticmethod
    def put(a, dtype=np.float64):
        return None if a is None else np.ascontiguousarray(a, dtype=dtype)

    @staticmethod
    def empty(shape, dtype=np.float64):
        return np.empty(shape, dtype=dtype)

    @staticmethod
    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)


class _Device:
    mem = _lib.DLM_MEM_DEVICE

    def __init__(self, device):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", device)

    def put(self, a, dtype=np.float64):
        if a is None:
            return None
        t = self.torch
        if isinstance(a, t.Tensor):
            want = t.float64 if dtype == np.float64 else t.int32
            return a.to(device=self.device, dtype=want).contiguous()
        return t.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=self.device)

    def empty(self, shape, dtype=np.float64):
        t = self.torch
        return t.empty(shape, dtype=t.float64 if dtype == np.float64 else t.int8 if dtype == np.int8 else t.int32, device=self.device)

    @staticmethod
    def ptr(a):
        return None if a is None else ctypes.c_void_p(a.data_ptr())


class Engine:
    """One engine per GPU (not thread-safe), mirroring `dlm_engine`."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.dlm_engine_create(int(device), ctypes.byref(h))
        if rc != 0:
            raise EngineError(f"dlm_engine_create(device={device}) failed with {rc}: no usable HIP device")
        self.h = h
        self.device = int(device)
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.dlm_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise EngineError(f"engine call failed ({rc}): {self.lib.dlm_last_error(self.h).decode()}")

    @property
    def last_variant(self) -> str:
        return self.lib.dlm_last_variant(self.h).decode()

    def set_stream(self, stream_ptr: Optional[int]):
        self._check(self.lib.dlm_engine_set_stream(self.h, ctypes.c_void_p(stream_ptr or 0)))

    def sync(self):
        self._check(self.lib.dlm_engine_sync(self.h))
        self._keep.clear()

    def _backend(self, y):
        if isinstance(y, np.ndarray) or y is None:
            return _Host()
        be = _Device(self.device)
        # Device mode takes torch tensors that were produced (or whose memory was last used) on torch's current stream,
        # while the engine launches on its own: order the engine's stream behind it (an event, no host wait).  The other
        # direction needs nothing for synchronous calls (the engine stream is drained on return); after DLM_OPT_ASYNC
        # calls sync() -- or stream_wait_engine() -- before torch touches the outputs.
        self._check(self.lib.dlm_engine_wait_stream(self.h, ctypes.c_void_p(be.torch.cuda.current_stream(be.device).cuda_stream or 0)))
        return be

    def stream_wait_engine(self, stream_ptr: Optional[int] = None):
        """Make `stream_ptr` (default: torch's current stream) wait for the engine work submitted so far."""
        if stream_ptr is None:
            import torch
            stream_ptr = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self.lib.dlm_stream_wait_engine(self.h, ctypes.c_void_p(stream_ptr or 0)))

    def _hold(self, flags, *objs):
        """Under DLM_OPT_ASYNC the kernels may still be reading the staged model / parameter tables and the inputs when
        the call returns: keep them alive until sync()."""
        if flags & _lib.OPT_ASYNC:
            self._keep.append(objs)

    def _call(self, name, be, flags, *args, keep=()):
        """The C call `name`(handle, *args), its return code checked.  args in the C order: where the symbol takes a data pointer an
        array of the backend crosses as its address and None as NULL; numbers cross as they are, and so do ctypes structures (the
        declared argtypes pass them by reference).  This is also the one place that keeps what the kernels may still read alive
        under DLM_OPT_ASYNC: every argument, and `keep` (the arrays behind a descriptor's pointers)."""
        self._hold(flags, args, keep)
        cargs, ptr = list(args), be.ptr
        for i in _POINTERS[name]:
            cargs[i] = ptr(cargs[i])
        self._check(getattr(self.lib, name)(self.h, *cargs))

    # -- engine-owned device buffers (what a caller without torch uses; also exercised by the tests) ----------------
    def buffer_alloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self._check(self.lib.dlm_buffer_alloc(self.h, int(nbytes), ctypes.byref(p)))
        return int(p.value)

    def buffer_free(self, ptr: int):
        self._check(self.lib.dlm_buffer_free(self.h, ctypes.c_void_p(ptr)))

    def buffer_upload(self, ptr: int, a: np.ndarray, offset: int = 0):
        a = np.ascontiguousarray(a)
        self._check(self.lib.dlm_buffer_upload(self.h, ctypes.c_void_p(ptr), int(offset), ctypes.c_void_p(a.ctypes.data), a.nbytes))

    def buffer_download(self, ptr: int, out: np.ndarray, offset: int = 0):
        assert out.flags["C_CONTIGUOUS"]
        self._check(self.lib.dlm_buffer_download(self.h, ctypes.c_void_p(ptr), int(offset), ctypes.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def mem_info(self):
        f, t = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.dlm_device_mem_info(self.h, ctypes.byref(f), ctypes.byref(t)))
        return int(f.value), int(t.value)

    def prepare(self, mat: MaterialisedModel, params, N: int, be, flags=0, seed=0, series_offset=0):
        """Build the descriptors; returns (model, params, opts, keepalive list)."""
        packed = pack_params(params, N) if not isinstance(params, tuple) else params
        V, vs, W, ws, m0, m0s, C0, c0s = packed[:8]
        vts, wts = (packed[8], packed[9]) if len(packed) > 8 else (0, 0)
        size = lambda a: a.numel() if hasattr(a, "numel") else np.size(a)     # (torch tensors: V_t / W_t streams kept on the device)
        if vts and size(V) // max(1, (N if vs else 1)) != mat.T * vts or wts and size(W) // max(1, (N if ws else 1)) != mat.T * wts:
            raise ValueError("time-varying V / W need one matrix per observation")
        items = dict(F=(mat.F, np.float64), G=(mat.G, np.float64), gi=(mat.g_index, np.int32), dt=(mat.dt, np.float64),
                     V=(V, np.float64), W=(W, np.float64), m0=(m0, np.float64), C0=(C0, np.float64))
        if isinstance(be, _Device) and not any(isinstance(a, be.torch.Tensor) for a, _ in items.values()):
            # device mode with a host-side model: ONE upload for all the small tables instead of eight
            parts, offs, pos = [], {}, 0
            for name, (a, dt) in items.items():
                if a is None:
                    continue
                b = np.ascontiguousarray(a, dtype=dt).reshape(-1).view(np.uint8)
                offs[name] = pos
                parts.append(b)
                pad = (-b.size) % 256
                if pad:
                    parts.append(np.zeros(pad, dtype=np.uint8))
                pos += b.size + pad
            host = np.concatenate(parts)
            # The staged tables of the call before are kept: the same bytes are not uploaded again, and the same MODEL bytes (F, G,
            # time grid -- the parameters may move, as in a Gibbs loop) let the engine reuse its analysis of their structure
            # (DLM_OPT_MODEL_UNCHANGED: two stream round trips per call less).  Not under DLM_OPT_ASYNC, whose tables may still be read.
            mend = offs.get("V", host.size)
            mkey = (mat.d, mat.p, mat.T, mat.n_g, mat.f_stride, host[:mend].tobytes())
            cache = getattr(self, "_staged", None)
            oflags = flags
            small = host.size <= (1 << 20)          # per-series or per-step parameter tables are not worth comparing: uploaded as before
            if not small:
                cache = None
            if cache is not None and not (flags & _lib.OPT_ASYNC) and cache["dev"] == be.device:
                if cache["mkey"] == mkey:   # compared byte for byte right here: the engine's device checksum of the promise is not needed
                    oflags |= _lib.OPT_MODEL_UNCHANGED | _lib.OPT_TRUST_MODEL_UNCHANGED
                blob = cache["blob"] if (cache["host"].size == host.size and np.array_equal(cache["host"], host)) else None
            else:
                blob = None
            if blob is None:
                blob = be.torch.as_tensor(host, device=be.device)
            self._staged = None if ((flags & _lib.OPT_ASYNC) or not small) else {"host": host, "blob": blob, "mkey": mkey, "dev": be.device}
            base = blob.data_ptr()
            bufs = {"blob": blob}
            P = lambda name: (base + offs[name]) if name in offs else None
            md = _lib.ModelDesc(mat.d, mat.p, mat.T, N, P("F"), mat.f_stride, P("G"), mat.n_g, P("gi"), P("dt"))
            pd = _lib.ParamsDesc(P("V"), vs, P("W"), ws, P("m0"), m0s, P("C0"), c0s, vts, wts)
            self._hold(flags, bufs)
            return md, pd, _options(be, oflags, seed, series_offset), bufs
        self._staged = None
        bufs = {name: be.put(a, dt) for name, (a, dt) in items.items()}
        P = lambda a: (be.ptr(a).value if a is not None else None)
        md = _lib.ModelDesc(mat.d, mat.p, mat.T, N, P(bufs["F"]), mat.f_stride, P(bufs["G"]), mat.n_g,
                            P(bufs["gi"]), P(bufs["dt"]))
        pd = _lib.ParamsDesc(P(bufs["V"]), vs, P(bufs["W"]), ws, P(bufs["m0"]), m0s, P(bufs["C0"]), c0s, vts, wts)
        self._hold(flags, bufs)
        return md, pd, _options(be, flags, seed, series_offset), bufs

    # -- entry points --------------------------------------------------------------
    def filter(self, mat, params, y, *, want_prior=False, want_fq=False, flags=0, out=None):
        """out: an existing record buffer [N][T+1][rec] to write into (its previous content must not matter)."""
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        rec = d + d * d
        yb = be.put(y).reshape(N, T, p)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags)
        filt = out if out is not None else be.empty((N, T + 1, self.lib.dlm_packed_record_doubles(d) if flags & _lib.OPT_PACKED_SYM else rec))
        out = _outputs(be, N, filt=filt, prior=(want_prior, (N, T + 1, rec)), fq=(want_fq, (N, T + 1, p + p * p)))
        self._call("dlm_filter_batch", be, flags, md, pd, yb, op, *out.values())
        return out

    def loglik(self, mat, params, y, *, flags=0):
        """Per-series prediction-error log-likelihood (dlm_loglik_batch); nothing but [N] numbers leaves the GPU."""
        be = self._backend(y)
        N = int(y.shape[0]); p, T = mat.p, mat.T
        yb = be.put(y).reshape(N, T, p)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags)
        out = _outputs(be, N, loglik=(True, (N,)))
        self._call("dlm_loglik_batch", be, flags, md, pd, yb, op, *out.values())
        return out

    def ar1_ffbs(self, y, v, sv, *, z=None, seed=0, series_offset=0, want_filt=True, want_theta=True, times=None):
        """Scalar AR(1) FFBS, one lane per series (dlm_ar1_ffbs_batch; FilterAr.scala:15-82).  y [N][T] (NaN = missing),
        v [N][T] or [T] per-step observation variances, sv [N][3] or [3] = (phi, mu, sigma_eta).  With `times` [T] it is
        the Ornstein-Uhlenbeck variant on that grid (dlm_ou_ffbs_batch; FilterOu.scala:7-79)."""
        be = self._backend(y)
        N, T = int(y.shape[0]), int(y.shape[1])
        yb = be.put(y).reshape(N, T)
        vv, v_stride = _strided(v, T, scalar=True)
        svv, sv_stride = _strided(sv, 3)
        vb, sb, zb = be.put(vv), be.put(svv), be.put(z)
        out = _outputs(be, N, filt=(want_filt, (N, T + 1, 2)), theta=(want_theta, (N, T + 1)))
        name, grid = ("dlm_ar1_ffbs_batch", ()) if times is None else ("dlm_ou_ffbs_batch", (be.put(times),))   # (a device tensor stays where it is)
        self._call(name, be, 0, N, T, *grid, yb, vb, v_stride, sb, sv_stride, zb, _options(be, 0, seed, series_offset), *out.values())
        return out

    def dinvgamma_step(self, d, p, stats, prior_v, prior_w, *, iteration, seed=0, series_offset=0):
        """GibbsSampling.dinvGammaStep on the device (dlm_dinvgamma_step_batch): stats [N][2p + d + 1] from an FFBS call
        -> (V [N][p*p], W [N][d*d]) dense diagonal matrices, ready as the next call's per-series parameters.
        prior_v / prior_w: (shape, scale) pairs or objects with .shape / .scale."""
        be = self._backend(stats)
        N = int(stats.shape[0])
        sb = be.put(stats)
        av, bv = (prior_v.shape, prior_v.scale) if hasattr(prior_v, "scale") else prior_v
        aw, bw = (prior_w.shape, prior_w.scale) if hasattr(prior_w, "scale") else prior_w
        V = be.empty((N, p * p)); W = be.empty((N, d * d))
        self._call("dlm_dinvgamma_step_batch", be, 0, int(d), int(p), N, sb, float(av), float(bv), float(aw), float(bw), int(iteration),
                   _options(be, 0, seed, series_offset), V, W)
        return V, W

    def studentt_step(self, mat, y, theta, stats, prior, scale, nu, *, iteration, accepted=None, seed=0, series_offset=0,
                      literal=False, want_loglik=True, flags=0, out=None):
        """One StudentT.step after its FFBS call (dlm_studentt_step_batch; StudentTGibbs.scala:182-212) for N chains.
        y [N][T] (or [N][T][1]; NaN = missing), theta [N][T+1][d] and stats [N][d + 3] of that FFBS call, scale [N] (s), nu [N]
        (int32); prior = (prior_nu_rate, prop_nu_size, prior_w_shape, prior_w_scale).  accepted [N] int32 is incremented in
        place (None: a fresh zero array).  Returns {"v" [N][T], "scale", "nu", "W" [N][d*d], "accepted", "loglik", "status"}: v is
        the next FFBS call's V stream (v_stride = T, v_tstride = 1).  literal=True: the reference's arithmetic (Q11-Q15).
        out: dict of existing buffers to write into ("v", "scale", "nu", "W"; scale / nu may be the inputs)."""
        be = self._backend(y)
        N, T, d = int(y.shape[0]), mat.T, mat.d
        if mat.p != 1:
            raise EngineError("the Student-t step is univariate: p must be 1")
        yb = be.put(y).reshape(N, T)
        tb, sb = be.put(theta), be.put(stats)
        scb, nub = be.put(scale), be.put(nu, np.int32)
        md, tables = _model_desc(be, mat, N, F=mat.F, f_stride=mat.f_stride, n_g=mat.n_g)
        res = _outputs(be, N, v=_out_or_empty(be, out, "v", (N, T)), scale=_out_or_empty(be, out, "scale", (N,)),
                       nu=_out_or_empty(be, out, "nu", (N,), np.int32), W=_out_or_empty(be, out, "W", (N, d * d)),
                       accepted=_counter(be, accepted, (N,)), loglik=(want_loglik, (N,)))
        op = _options(be, flags | (_lib.OPT_STUDENTT_LITERAL if literal else 0), seed, series_offset)
        self._call("dlm_studentt_step_batch", be, flags, md, yb, tb, sb, _as_prior(_lib.StudentTPrior, prior), scb, nub, int(iteration), op,
                   *res.values(), keep=tables)
        return res

    def sv_mixture(self, y, alpha, *, iteration, seed=0, series_offset=0, want_k=False, flags=0, out=None):
        """The mixture indicators of the stochastic-volatility sampler (dlm_sv_mixture_batch; StochasticVolatility.sampleKt,
        StochasticVolatility.scala:112-157) for N chains: y [N][T] (NaN = missing), alpha [N][T+1] as ar1_ffbs writes its theta.
        Returns {"ystar" [N][T], "v" [N][T], "k" [N][T] int8 or None, "status"}: ystar and v are the next ar1_ffbs call's y and v.
        alpha=None: the initial transform (ystar = log y^2 + 1.27, v = pi^2 / 2; no draw, no k).
        out: dict of existing buffers to write into ("ystar", "v", "k")."""
        be = self._backend(y)
        N, T = int(y.shape[0]), int(y.shape[1])
        yb = be.put(y).reshape(N, T)
        ab = be.put(alpha)
        if ab is not None and tuple(ab.shape) != (N, T + 1):
            raise EngineError(f"alpha must be [N][T+1] = {(N, T + 1)}, got {tuple(ab.shape)}")
        res = _outputs(be, N, ystar=_out_or_empty(be, out, "ystar", (N, T)), v=_out_or_empty(be, out, "v", (N, T)),
                       k=_out_or_empty(be, out, "k", (N, T), np.int8) if want_k and ab is not None else None)
        self._call("dlm_sv_mixture_batch", be, flags, N, T, yb, ab, int(iteration), _options(be, flags, seed, series_offset), *res.values())
        return res

    def sv_params(self, alpha, sv, prior, *, iteration, accepted=None, seed=0, series_offset=0, flags=0, out=None):
        """phi, mu, sigma of the stochastic-volatility sampler given the state draw (dlm_sv_params_batch; samplePhiConjugate or
        samplePhi, sampleMu, sampleSigma) for N chains: alpha [N][T+1], sv [N][3] = (phi, mu, sigma).  prior: a _lib.SvPrior, or its ten
        fields in order (phi_update, literal, phi_a, phi_b, mu_mean, mu_sd, sigma_shape, sigma_scale, prop_lambda, prop_tau).
        accepted [N] int32 is incremented in place (None: a fresh zero array).  Returns {"sv" [N][3], "accepted", "status"}.
        out: dict with an existing "sv" buffer to write into (it may be the input)."""
        return self._sv_params(None, alpha, sv, prior, iteration, accepted, seed, series_offset, flags, out)

    def sv_ou_params(self, times, alpha, sv, prior, *, iteration, accepted=None, seed=0, series_offset=0, flags=0, out=None):
        """phi, sigma, mu of the stochastic-volatility sampler with Ornstein-Uhlenbeck log-volatility given the state draw
        (dlm_sv_ou_params_batch; samplePhiOu, sampleSigmaMetropOu, sampleMuOu in stepOu's order) for N chains: times [T] shared by the
        batch, alpha [N][T+1] as ar1_ffbs(times=...) writes its theta, sv [N][3] = (phi, mu, sigma) with phi the mean-reversion rate.
        prior: a _lib.SvOuPrior, or its eleven fields in order (literal, phi_a, phi_b, mu_mean, mu_sd, sigma_shape, sigma_scale,
        prop_lambda, prop_tau, delta_sigma, delta_mu).  accepted [N][3] int32 (phi, sigma, mu) is incremented in place (None: a fresh
        zero array).  Returns {"sv" [N][3], "accepted", "status"}.  out: dict with an existing "sv" buffer to write into (it may be
        the input)."""
        return self._sv_params(times, alpha, sv, prior, iteration, accepted, seed, series_offset, flags, out)

    def _sv_params(self, times, alpha, sv, prior, iteration, accepted, seed, series_offset, flags, out):
        """sv_params (times=None: one acceptance counter per series) and sv_ou_params (its grid; three counters per series)."""
        ou = times is not None
        be = self._backend(alpha)
        N, T = int(alpha.shape[0]), int(alpha.shape[1]) - 1
        ab, sb, tb = be.put(alpha), be.put(sv), be.put(times)
        if ou and tuple(tb.shape) != (T,):
            raise EngineError(f"times must be [T] = {(T,)}, got {tuple(tb.shape)}")
        if tuple(sb.shape) != (N, 3):
            raise EngineError(f"sv must be [N][3] = {(N, 3)}, got {tuple(sb.shape)}")
        pr = _as_prior(_lib.SvOuPrior if ou else _lib.SvPrior, prior)
        res = _outputs(be, N, sv=_out_or_empty(be, out, "sv", (N, 3)), accepted=_counter(be, accepted, (N, 3) if ou else (N,)))
        name, grid = ("dlm_sv_ou_params_batch", (tb,)) if ou else ("dlm_sv_params_batch", ())
        self._call(name, be, flags, N, T, *grid, ab, sb, pr, int(iteration), _options(be, flags, seed, series_offset), *res.values())
        return res

    def sv_knots(self, y, alpha, sv, knots, *, iteration, accepted=None, seed=0, series_offset=0, out=None):
        """One sweep of the knot block sampler over the log-volatility paths of N chains (dlm_sv_knots_batch;
        StochasticVolatilityKnots.sampleState, StochVolKnots.scala:74-176): y [N][T] (NaN = missing), alpha [N][T+1] as ar1_ffbs writes
        its theta, sv [N][3] or [3] = (phi, mu, sigma), knots [B+1] int32 shared by the batch (0 = knots[0] < ... < knots[B] = T + 1;
        stochvol.sample_knots draws them).  Every block is proposed from the Gaussian approximation log y^2 + 1.27 ~ N(alpha, pi^2 / 2)
        given its neighbours and accepted by a Metropolis step against the exact likelihood; even blocks first, then odd blocks.
        accepted [N] int32 is incremented in place by the number of accepted blocks (None: a fresh zero array).  Returns {"alpha"
        [N][T+1], "accepted", "status"}: alpha is a new buffer, the input is left as it is -- unless out["alpha"] is given: the sweep
        runs in that buffer (it may be the input itself)."""
        be = self._backend(y)
        N, T = int(y.shape[0]), int(y.shape[1])
        yb = be.put(y).reshape(N, T)
        ab = be.put(alpha)
        if tuple(ab.shape) != (N, T + 1):
            raise EngineError(f"alpha must be [N][T+1] = {(N, T + 1)}, got {tuple(ab.shape)}")
        svv, sv_stride = _strided(sv, 3)
        if tuple(svv.shape) not in ((3,), (N, 3)):
            raise EngineError(f"sv must be [3] or [N][3] = {(N, 3)}, got {tuple(svv.shape)}")
        sb, kb = be.put(svv), be.put(knots, np.int32)
        if kb.ndim != 1 or int(kb.shape[0]) < 2:
            raise EngineError(f"knots must be [B+1] with B >= 1, got the shape {tuple(kb.shape)}")
        new = _out_or_empty(be, out, "alpha", (N, T + 1))
        if new is not ab:
            if tuple(new.shape) != (N, T + 1):
                raise EngineError(f"out['alpha'] must be [N][T+1] = {(N, T + 1)}, got {tuple(new.shape)}")
            if isinstance(new, np.ndarray):
                np.copyto(new, ab)
            else:
                new.copy_(ab)
                be = self._backend(y)   # (the copy ran on torch's stream: the engine's waits for it)
        res = _outputs(be, N, alpha=new, accepted=_counter(be, accepted, (N,)))
        self._call("dlm_sv_knots_batch", be, 0, N, T, yb, kb, int(kb.shape[0]) - 1, sb, sv_stride, int(iteration),
                   _options(be, 0, seed, series_offset), *res.values())
        return res

    def fsv_factors(self, y, beta, v, alpha, *, iteration, seed=0, series_offset=0, literal=False, flags=0, out=None):
        """The factor draw of the factor stochastic-volatility sampler (dlm_fsv_factors_batch; FactorSv.sampleFactors,
        FactorSv.scala:168-186) for N panels: y [N][T][p] (NaN = missing; a partially missing time is wholly missing), beta [N][p][k],
        v [N][p] the diagonal of the observation variance, alpha [N][k][T+1] the factors' log-volatilities (alpha[..][t+1] belongs to
        y[t]) or None: unit factor variances (initialiseFactors).  Returns {"f" [N][k][T], "status"}: f viewed as [N k][T] is the y of
        sv_mixture, NaN where the time is missing.  literal=True: the reference's draw (Q27).  out: dict with an existing "f" buffer."""
        be = self._backend(y)
        if y.ndim != 3 or beta.ndim != 3:
            raise EngineError("y must be [N][T][p] and beta [N][p][k]")
        N, T, p, k = int(y.shape[0]), int(y.shape[1]), int(y.shape[2]), int(beta.shape[2])
        yb, bb, vb, ab = be.put(y), be.put(beta), be.put(v), be.put(alpha)
        if tuple(bb.shape) != (N, p, k) or tuple(vb.shape) != (N, p):
            raise EngineError(f"beta must be [N][p][k] = {(N, p, k)} and v [N][p] = {(N, p)}, got {tuple(bb.shape)} and {tuple(vb.shape)}")
        if ab is not None and tuple(ab.shape) != (N, k, T + 1):
            raise EngineError(f"alpha must be [N][k][T+1] = {(N, k, T + 1)}, got {tuple(ab.shape)}")
        res = _outputs(be, N, f=_out_or_empty(be, out, "f", (N, k, T)))
        self._call("dlm_fsv_factors_batch", be, flags, N, T, p, k, yb, bb, vb, ab, 1 if literal else 0, int(iteration),
                   _options(be, flags, seed, series_offset), *res.values())
        return res

    def fsv_loadings(self, y, f, beta, prior, *, iteration, seed=0, series_offset=0, v=None, flags=0, out=None):
        """sigma^2 and the loading matrix of the factor stochastic-volatility sampler given the factors (dlm_fsv_loadings_batch;
        FactorSv.sampleSigmaUni, :516-541, then sampleBeta, :253-333) for N panels: y [N][T][p], f [N][k][T] as fsv_factors writes it,
        beta [N][p][k] the current loadings.  prior: a _lib.FsvPrior, or its five fields in order (literal, beta_mean, beta_sd,
        sigma_shape, sigma_scale).  v [N][p] (optional): what a panel without an observed time keeps.  Returns {"beta" [N][p][k],
        "v" [N][p] (sigma^2 in every entry), "status"}.  out: dict of existing "beta" / "v" buffers (they may be the inputs)."""
        be = self._backend(y)
        if y.ndim != 3 or beta.ndim != 3:
            raise EngineError("y must be [N][T][p] and beta [N][p][k]")
        N, T, p, k = int(y.shape[0]), int(y.shape[1]), int(y.shape[2]), int(beta.shape[2])
        yb, fb, bb, vb = be.put(y), be.put(f), be.put(beta), be.put(v)
        if tuple(bb.shape) != (N, p, k) or tuple(fb.shape) != (N, k, T):
            raise EngineError(f"beta must be [N][p][k] = {(N, p, k)} and f [N][k][T] = {(N, k, T)}, got {tuple(bb.shape)} and {tuple(fb.shape)}")
        if vb is not None and tuple(vb.shape) != (N, p):
            raise EngineError(f"v must be [N][p] = {(N, p)}, got {tuple(vb.shape)}")
        pr = _as_prior(_lib.FsvPrior, prior)
        res = _outputs(be, N, beta=_out_or_empty(be, out, "beta", (N, p, k)), v=_out_or_empty(be, out, "v", (N, p)))
        self._call("dlm_fsv_loadings_batch", be, flags, N, T, p, k, yb, fb, bb, vb, pr, int(iteration),
                   _options(be, flags, seed, series_offset), *res.values())
        return res

    def dlmfsv_center(self, mat, y, theta, *, flags=0, out=None):
        """The panel centred on the DLM's mean (dlm_dlmfsv_center_batch; factorObs, DlmFsv.scala:173-185) for N panels:
        r[t] = y[t] - F_t^T theta[t+1], y [N][T][p] (a NaN stays NaN), theta [N][T+1][d] as ffbs writes it, mat the materialised model
        (its F, time-invariant or per time).  Returns {"r" [N][T][p], "status"}.  out: dict with an existing "r" buffer."""
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        yb, tb = be.put(y), be.put(theta)
        if tuple(yb.shape) != (N, T, p) or tuple(tb.shape) != (N, T + 1, d):
            raise EngineError(f"y must be [N][T][p] = {(N, T, p)} and theta [N][T+1][d] = {(N, T + 1, d)}, got {tuple(yb.shape)} and {tuple(tb.shape)}")
        md, tables = _model_desc(be, mat, N, F=mat.F, f_stride=mat.f_stride)
        res = _outputs(be, N, r=_out_or_empty(be, out, "r", (N, T, p)))
        self._call("dlm_dlmfsv_center_batch", be, flags, md, yb, tb, _options(be, flags), *res.values(), keep=tables)
        return res

    def dlmfsv_impute(self, r, beta, v, alpha, *, iteration, seed=0, series_offset=0, flags=0, out=None):
        """The missing components of the partially missing times of a centred panel, drawn given the observed ones
        (dlm_dlmfsv_impute_batch): r [N][T][p] (NaN = missing), beta [N][p][k], v [N][p], alpha [N][k][T+1].  Times with
        all or none of their components finite are copied.  Returns {"r" [N][T][p], "status"}.  out: dict with an existing "r" buffer
        (it may be r itself)."""
        be = self._backend(r)
        if r.ndim != 3 or beta.ndim != 3:
            raise EngineError("r must be [N][T][p] and beta [N][p][k]")
        N, T, p, k = int(r.shape[0]), int(r.shape[1]), int(r.shape[2]), int(beta.shape[2])
        rb, bb, vb, ab = be.put(r), be.put(beta), be.put(v), be.put(alpha)
        if tuple(bb.shape) != (N, p, k) or tuple(vb.shape) != (N, p) or tuple(ab.shape) != (N, k, T + 1):
            raise EngineError(f"beta must be [N][p][k] = {(N, p, k)}, v [N][p] = {(N, p)} and alpha [N][k][T+1] = {(N, k, T + 1)}, got "
                              f"{tuple(bb.shape)}, {tuple(vb.shape)} and {tuple(ab.shape)}")
        res = _outputs(be, N, r=_out_or_empty(be, out, "r", (N, T, p)))
        self._call("dlm_dlmfsv_impute_batch", be, flags, N, T, p, k, rb, bb, vb, ab, int(iteration), _options(be, flags, seed, series_offset),
                   *res.values())
        return res

    def dlmfsv_variance(self, beta, v, alpha, *, flags=0, out=None):
        """The observation-variance stream of the DLM with factor stochastic-volatility noise (dlm_dlmfsv_variance_batch;
        DlmFsvSystem.calculateVariance, DlmFsvSystem.scala:126-131) for N panels: V[n][t] = beta diag(exp(alpha[.., t+1])) beta^T + diag(v),
        beta [N][p][k], v [N][p], alpha [N][k][T+1].  Returns {"V" [N][T][p*p] (symmetric bit for bit: the V of ffbs with
        v_stride = T p p, v_tstride = p p), "status"}.  out: dict with an existing "V" buffer."""
        be = self._backend(beta)
        if beta.ndim != 3 or alpha.ndim != 3:
            raise EngineError("beta must be [N][p][k] and alpha [N][k][T+1]")
        N, p, k, T = int(beta.shape[0]), int(beta.shape[1]), int(beta.shape[2]), int(alpha.shape[2]) - 1
        bb, vb, ab = be.put(beta), be.put(v), be.put(alpha)
        if tuple(vb.shape) != (N, p) or tuple(ab.shape) != (N, k, T + 1):
            raise EngineError(f"v must be [N][p] = {(N, p)} and alpha [N][k][T+1] = {(N, k, T + 1)}, got {tuple(vb.shape)} and {tuple(ab.shape)}")
        res = _outputs(be, N, V=_out_or_empty(be, out, "V", (N, T, p * p)))
        self._call("dlm_dlmfsv_variance_batch", be, flags, N, T, p, k, bb, vb, ab, _options(be, flags), *res.values())
        return res

    def dlmfsvsys_innovations(self, mat, theta, *, flags=0, out=None):
        """The state's innovations (dlm_dlmfsvsys_innovations_batch; factorState, DlmFsvSystem.scala:109-117) for N panels:
        w[t] = theta[t+1] - G theta[t], theta [N][T+1][d] as ffbs writes it, mat the materialised model (its one G; a table of G or an
        irregular grid is refused by the call).  Returns {"w" [N][T][d], "status"}.  out: dict with an existing "w" buffer (not theta)."""
        be = self._backend(theta)
        N = int(theta.shape[0]); d, T = mat.d, mat.T
        tb = be.put(theta)
        if tuple(tb.shape) != (N, T + 1, d):
            raise EngineError(f"theta must be [N][T+1][d] = {(N, T + 1, d)}, got {tuple(tb.shape)}")
        md, tables = _model_desc(be, mat, N, G=mat.G, n_g=mat.n_g, g_index=mat.g_index, dt=mat.dt)
        res = _outputs(be, N, w=_out_or_empty(be, out, "w", (N, T, d)))
        self._call("dlm_dlmfsvsys_innovations_batch", be, flags, md, tb, _options(be, flags), *res.values(), keep=tables)
        return res

    def sv_paths(self, sv, horizon, n_paths, *, alpha0=None, iteration=0, seed=0, series_offset=0, flags=0, out=None):
        """Future log-volatility paths of the factor stochastic-volatility models (dlm_sv_paths; StochasticVolatility.stepState): sv
        [N][k][3] = (phi, mu, sigma_eta), alpha0 [N][k] the start of every path of a row or None: a draw from the stationary law.  Returns
        {"alpha" [N][R][k][H+1] (entry 0 the start; viewed as [N R][k][H+1] the alpha of dlmfsv_variance with T = H), "status"}; path r of
        row n is a pure function of (seed, series_offset + n, iteration, r), so a call with more paths or other rows repeats it.  A row
        with |phi| >= 1 or sigma <= 0 has DLM_ST_NOT_PD, one with a non-finite input DLM_ST_NONFINITE, and NaN paths.  out: dict with an
        existing "alpha" buffer."""
        if len(sv.shape) != 3 or int(sv.shape[2]) != 3:
            raise EngineError(f"sv must be [N][k][3], got the shape {tuple(sv.shape)}")
        N, k, H, R = int(sv.shape[0]), int(sv.shape[1]), int(horizon), int(n_paths)
        check_sv_paths_shape(k, H, R)
        be = self._backend(sv)
        sb, ab = be.put(sv), be.put(alpha0)
        if ab is not None and tuple(ab.shape) != (N, k):
            raise EngineError(f"alpha0 must be [N][k] = {(N, k)}, got {tuple(ab.shape)}")
        res = _outputs(be, N, alpha=_out_or_empty(be, out, "alpha", (N, R, k, H + 1)))
        self._call("dlm_sv_paths", be, flags, N, k, H, R, sb, ab, int(iteration), _options(be, flags, seed, series_offset), *res.values())
        return res

    def gaussian_mixture_summary(self, N, C, H, p, *, fq=None, Q=None, f=None, q_strides=None, f_strides=None, probs=(), flags=0, out=None):
        """Mean, total covariance and exact marginal quantiles of the equal-weight mixture of C Gaussians N(f_c, Q_c) per row and time
        (dlm_gaussian_mixture_summary), read in place:
          fq   the records [N C][H+1][p + p p] of filter(..., want_fq=True) on N C rows (record 0 is skipped), or
          Q    [N C][H][p p] (a variance stream of dlmfsv_variance as it is) with f [N C][H][p] or None (zero means);
               q_strides / f_strides = (row, component, time) in doubles say where a differently laid out Q / f has its records.
        probs: up to 8 probabilities inside (0, 1).  Returns {"mean" [N][H][p], "cov" [N][H][p p] (symmetric bit for bit), "quant"
        [N][H][p][nq] or None, "status" [N]}.  A quantile is the root of the mixture's CDF bracketed to adjacent doubles (bisection
        safeguarding Newton; no sampling).  A row with a Q_ii that is not positive and finite has DLM_ST_NOT_PD, with a non-finite f
        DLM_ST_NONFINITE, and NaN in that cell.  out: dict of existing "mean" / "cov" / "quant" buffers."""
        N, C, H, p = int(N), int(C), int(H), int(p)
        pr = check_mixture_shape(N, C, H, p, probs)
        rec, pp = p + p * p, p * p
        if (fq is None) == (Q is None):
            raise EngineError("give either fq (the filter's records) or Q (with an optional f)")
        be = self._backend(fq if fq is not None else Q)
        size = lambda a: int(a.numel() if hasattr(a, "numel") else a.size)
        if fq is not None:
            flat = be.put(fq).reshape(-1)
            if size(flat) != N * C * (H + 1) * rec:
                raise EngineError(f"fq must hold [N C][H+1][p + p p] = {(N * C, H + 1, rec)} doubles, got {size(flat)}")
            fb, qb = flat[rec:], flat[rec + p:]
            fs = qs = (C * (H + 1) * rec, (H + 1) * rec, rec)
        else:
            qb = be.put(Q).reshape(-1)
            fb = None if f is None else be.put(f).reshape(-1)
            qs = tuple(int(s) for s in q_strides) if q_strides is not None else (C * H * pp, H * pp, pp)
            fs = tuple(int(s) for s in f_strides) if f_strides is not None else (C * H * p, H * p, p)
            if len(qs) != 3 or len(fs) != 3 or min(qs + fs) < 0:
                raise EngineError("q_strides and f_strides are (row, component, time) strides in doubles, none negative")
            extent = lambda s, last: (N - 1) * s[0] + (C - 1) * s[1] + (H - 1) * s[2] + last
            if size(qb) < extent(qs, pp) or (fb is not None and size(fb) < extent(fs, p)):
                raise EngineError("Q / f is smaller than what N, C, H, p and the strides reach")
        nq = len(pr)
        res = _outputs(be, N, mean=_out_or_empty(be, out, "mean", (N, H, p)), cov=_out_or_empty(be, out, "cov", (N, H, pp)),
                       quant=_out_or_empty(be, out, "quant", (N, H, p, nq)) if nq else None)
        desc = _lib.MixtureDesc(N, C, H, p, nq, *fs, *qs)
        prc = (ctypes.c_double * nq)(*pr) if nq else None          # a host array whatever the backend: the call reads it before it returns
        self._call("dlm_gaussian_mixture_summary", be, flags, desc, fb, qb, prc, _options(be, flags), *res.values())
        return res

    def particle_filter(self, mat, params, y, *, family, n_particles, n0=-1, literal=False, obs_param=None, iteration=0, seed=0,
                        series_offset=0, flags=0, want_mean=True, want_ess=True, want_cloud=True, want_weights=True,
                        resample=_lib.RESAMPLE_MULTINOMIAL, mh_steps=0):
        """Bootstrap particle filter of a dynamic generalised linear model (dlm_pf_batch, and dlm_pf_resampled under any scheme but the multinomial one; ParticleFilter.step, ParticleFilter.scala:38-61) for
        N series of P = n_particles particles: y [N][T] (NaN = missing), params one DlmParameters, N of them or the packed tuple of
        pack_params (per-series parameters: what a particle-marginal Metropolis step evaluates), family one of _lib.OBS_*, obs_param [N] or a
        scalar: the degrees of freedom of OBS_STUDENTT.  n0: resample when ESS < n0 (negative: floor(P / 5), ParticleFilter.likelihood).
        literal=True: the reference's arithmetic (Q37-Q39).  resample: one of _lib.RESAMPLE_* (multinomial: dlm_pf_batch bit for bit;
        stratified and systematic: unbiased too, with a smaller variance of ll; Metropolis with mh_steps = 1..PF_MAX_MH_STEPS chain steps:
        BIASED, include/dlm_engine.h says how).  Returns {"ll" [N], "mean" [N][T][d], "ess" [N][T], "cloud" [N][d][P],
        "weights" [N][P], "status" [N]}; the optional ones are None when not wanted.  A series with a status bit has ll = -inf."""
        scheme, b = check_pf_resample(resample, mh_steps)
        be = self._backend(y)
        d, T, P = _pf_shape(mat, n_particles, family)
        N, yb, ob = _pf_data(be, y, T, family, obs_param)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride or pd.w_tstride:
            raise EngineError("the particle filter takes time-invariant V and W")
        out = _outputs(be, N, ll=(True, (N,)), mean=(want_mean, (N, T, d)), ess=(want_ess, (N, T)), cloud=(want_cloud, (N, d, P)),
                       weights=(want_weights, (N, P)))
        desc = _lib.PfDesc(int(family), P, int(n0), 1 if literal else 0)
        if scheme == _lib.RESAMPLE_MULTINOMIAL:          # (dlm_pf_batch IS dlm_pf_resampled with this scheme: one host path, the same bits)
            self._call("dlm_pf_batch", be, flags, md, pd, desc, ob, yb, int(iteration), op, *out.values())
        else:
            self._call("dlm_pf_resampled", be, flags, md, pd, desc, _lib.ResampleDesc(scheme, b), ob, yb, int(iteration), op, *out.values())
        return out

    def pf_forecast(self, mat, params, y, *, family, n_particles, ranks=(), cloud=None, weights=None, slot_offset=0, literal=False,
                    obs_param=None, iteration=0, seed=0, series_offset=0, flags=0, want_draws=False, want_mean=True, want_cloud=True,
                    want_weights=False):
        """Posterior-predictive forecast of a dynamic generalised linear model from a particle cloud (dlm_pf_forecast_particles;
        Dglm.forecastParticles, Dglm.scala:297-331) for N series of P = n_particles particles: mat describes the H forecast steps (dt[0] the
        gap from the time of the cloud), y [N][H] with NaN = "forecast, do not update"; an observed step updates and resamples the cloud.
        cloud [N][d][P]: the cloud to start from (None: drawn from (m0, C0) as particle_filter draws it), weights [N][P] its weights (None:
        equal; given: the cloud is resampled once at entry).  ranks: up to 8 order statistics of the P draws of a time, 0 <= rank < P.
        slot_offset: step h draws from the Philox slot slot_offset + h (the number of steps filtered so far continues their stream).
        params, family, obs_param, literal as in particle_filter.  Returns {"fmean" [N][H] the mean of the draws, "fquant" [N][H][len(ranks)]
        their order statistics, "draws" [N][H][P], "ll" [N], "mean" [N][H][d] the filtering mean, "cloud" [N][d][P], "weights" [N][P],
        "status" [N]}; the optional ones are None when not wanted.  A series with a status bit has ll = -inf and NaN from the failing step on."""
        d, T, P = _pf_shape(mat, n_particles, family)
        rk = check_pf_ranks(ranks, P)
        if weights is not None and cloud is None:
            raise EngineError("weights need the cloud they weigh: pass cloud too")
        if not 0 <= int(slot_offset) <= _lib.PF_MAX_T - T:
            raise EngineError(f"slot_offset + the number of steps must stay within {_lib.PF_MAX_T} (the Philox counter's slot field), got {slot_offset} + {T}")
        be = self._backend(y)
        N, yb, ob = _pf_data(be, y, T, family, obs_param)
        cb, wb = be.put(cloud), be.put(weights)
        if cb is not None and tuple(cb.shape) != (N, d, P):
            raise EngineError(f"cloud must be [N][d][P] = {(N, d, P)}, got {tuple(cb.shape)}")
        if wb is not None and tuple(wb.shape) != (N, P):
            raise EngineError(f"weights must be [N][P] = {(N, P)}, got {tuple(wb.shape)}")
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride or pd.w_tstride:
            raise EngineError("the particle forecast takes time-invariant V and W")
        out = _outputs(be, N, fmean=(True, (N, T)), fquant=(bool(rk), (N, T, len(rk))), draws=(want_draws, (N, T, P)), ll=(True, (N,)),
                       mean=(want_mean, (N, T, d)), cloud=(want_cloud, (N, d, P)), weights=(want_weights, (N, P)))
        desc = _lib.PfForecastDesc(int(family), P, 1 if literal else 0, len(rk), int(slot_offset))
        rkc = (ctypes.c_int32 * len(rk))(*rk) if rk else None          # a host array whatever the backend: the call reads it before it returns
        self._call("dlm_pf_forecast_particles", be, flags, md, pd, desc, ob, rkc, cb, wb, yb, int(iteration), op, *out.values())
        return out

    def storvik_filter(self, mat, params, y, prior_w, *, family, n_particles, prior_v=None, learn_v=None, n0=-1, literal=False,
                       obs_param=None, iteration=0, seed=0, series_offset=0, flags=0, want_mean=True, want_ess=True, want_scale_mean=True,
                       want_cloud=True, want_weights=True, want_scales=True):
        """Storvik filter of a dynamic generalised linear model (dlm_storvik_batch; StorvikFilter.step, Storvik.scala:105-159): the particle
        filter of `particle_filter` with the diagonal of W -- and with learn_v (default: the Gaussian family) V -- learned online from
        InverseGamma priors.  prior_w: (shape, scale) per component, [d][2] shared or [N][d][2] per series; prior_v: [2] or [N][2] (needed
        with learn_v).  params as in particle_filter: its W is not read, its V only without learn_v.  literal=True: Q39 and Q43.
        Returns {"ll" [N], "mean" [N][T][d], "ess" [N][T], "scale_mean" [N][T][d+1], "cloud" [N][d][P], "weights" [N][P],
        "scales" [N][d+1][P], "status" [N]}; the optional ones are None when not wanted, the entries d of scale_mean and scales NaN
        without learn_v."""
        be = self._backend(y)
        d, T, P = _pf_shape(mat, n_particles, family)
        learn_v = family == _lib.OBS_GAUSSIAN if learn_v is None else bool(learn_v)
        if learn_v and family != _lib.OBS_GAUSSIAN:
            raise EngineError("learn_v needs OBS_GAUSSIAN: the InverseGamma statistic of V is conjugate for the Gaussian family only")
        if learn_v and prior_v is None:
            raise EngineError("learn_v needs prior_v = (shape, scale)")
        N, yb, ob = _pf_data(be, y, T, family, obs_param)
        pvb, pv_stride, pwb, pw_stride = _pf_priors(be, prior_w, prior_v, learn_v, N, d)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride and not learn_v:
            raise EngineError("the Storvik filter takes a time-invariant V")
        out = _outputs(be, N, ll=(True, (N,)), mean=(want_mean, (N, T, d)), ess=(want_ess, (N, T)), scale_mean=(want_scale_mean, (N, T, d + 1)),
                       cloud=(want_cloud, (N, d, P)), weights=(want_weights, (N, P)), scales=(want_scales, (N, d + 1, P)))
        desc = _lib.StorvikDesc(int(family), P, int(n0), 1 if literal else 0, 1 if learn_v else 0)
        self._call("dlm_storvik_batch", be, flags, md, pd, desc, pvb, pv_stride, pwb, pw_stride, ob, yb, int(iteration), op, *out.values())
        return out

    def lw_filter(self, mat, params, y, prior_w, *, family, n_particles, a, prior_v=None, learn_v=None, n0=-1, literal=False,
                  obs_param=None, iteration=0, seed=0, series_offset=0, flags=0, want_mean=True, want_ess=True, want_psi_mean=True,
                  want_psi_var=True, want_cloud=True, want_weights=True, want_psi=True):
        """Liu-West filter of a dynamic generalised linear model (dlm_lw_batch; LiuAndWestFilter.step, LiuAndWest.scala:47-81): an auxiliary
        particle filter whose particles carry their own log-variances -- log W_kk, and with learn_v (default: the family is Gaussian,
        Student-t or Beta) log V -- shrunk by `a` (0 < a <= 1) and jittered at every step.  prior_w: (mean, sd) of log W_kk per component,
        [d][2] shared or [N][d][2] per series; prior_v: [2] or [N][2] (needed with learn_v); sd = 0: a known variance.  params as in
        particle_filter: its W is not read, its V only without learn_v.  literal=True: Q39, Q50 and Q51.
        Returns {"ll" [N], "mean" [N][T][d], "ess" [N][T], "psi_mean" [N][T][d+1], "psi_var" [N][T][d+1], "cloud" [N][d][P],
        "weights" [N][P], "psi" [N][d+1][P], "status" [N]}; the optional ones are None when not wanted, the entries d of psi_mean, psi_var
        and psi NaN without learn_v."""
        be = self._backend(y)
        d, T, P = _pf_shape(mat, n_particles, family)
        scale_family = family in (_lib.OBS_GAUSSIAN, _lib.OBS_STUDENTT, _lib.OBS_BETA)
        learn_v = scale_family if learn_v is None else bool(learn_v)
        if learn_v and not scale_family:
            raise EngineError("learn_v needs OBS_GAUSSIAN, OBS_STUDENTT or OBS_BETA: the families whose v is a positive scale")
        if learn_v and prior_v is None:
            raise EngineError("learn_v needs prior_v = (mean, sd) of log V")
        check_shrinkage(a)
        N, yb, ob = _pf_data(be, y, T, family, obs_param)
        pvb, pv_stride, pwb, pw_stride = _pf_priors(be, prior_w, prior_v, learn_v, N, d)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride and not learn_v:
            raise EngineError("the Liu-West filter takes a time-invariant V")
        out = _outputs(be, N, ll=(True, (N,)), mean=(want_mean, (N, T, d)), ess=(want_ess, (N, T)), psi_mean=(want_psi_mean, (N, T, d + 1)),
                       psi_var=(want_psi_var, (N, T, d + 1)), cloud=(want_cloud, (N, d, P)), weights=(want_weights, (N, P)),
                       psi=(want_psi, (N, d + 1, P)))
        desc = _lib.LwDesc(int(family), P, int(n0), 1 if literal else 0, 1 if learn_v else 0, float(a))
        self._call("dlm_lw_batch", be, flags, md, pd, desc, pvb, pv_stride, pwb, pw_stride, ob, yb, int(iteration), op, *out.values())
        return out

    def rb_filter(self, mat, params, y, prior_w, *, n_particles, a, prior_v=None, learn_v=True, n0=-1, literal=False, iteration=0, seed=0,
                  series_offset=0, flags=0, want_mean=True, want_cov=True, want_ess=True, want_psi_mean=True, want_psi_var=True,
                  want_means=True, want_covs=True, want_weights=True, want_psi=True):
        """Rao-Blackwellised particle filter of a Gaussian DLM (dlm_rb_batch; RaoBlackwellFilter.scala): the Liu-West filter of `lw_filter`
        whose particles carry the Kalman mean and covariance of the state given their own log-variances in place of a drawn state.
        prior_w, prior_v, a, n0 and params as in lw_filter (sd = 0: a known variance; with every variance known the filter is the Kalman
        filter).  literal=True: Q50, Q57 and Q58.  Returns {"ll" [N], "mean" [N][T][d], "cov" [N][T][d][d] (the mixture covariance),
        "ess" [N][T], "psi_mean", "psi_var" [N][T][d+1], "means" [N][d][P], "covs" [N][d(d+1)/2][P] (the lower triangles by rows),
        "weights" [N][P], "psi" [N][d+1][P], "status" [N]}; the optional ones are None when not wanted, the entries d of psi_mean, psi_var
        and psi NaN without learn_v."""
        be = self._backend(y)
        d, T, P = _pf_shape(mat, n_particles, _lib.OBS_GAUSSIAN)
        check_rb_lds(d, P)
        learn_v = bool(learn_v)
        if learn_v and prior_v is None:
            raise EngineError("learn_v needs prior_v = (mean, sd) of log V")
        check_shrinkage(a)
        N, yb, _ = _pf_data(be, y, T, _lib.OBS_GAUSSIAN, None)
        pvb, pv_stride, pwb, pw_stride = _pf_priors(be, prior_w, prior_v, learn_v, N, d)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride and not learn_v:
            raise EngineError("the Rao-Blackwellised filter takes a time-invariant V")
        out = _outputs(be, N, ll=(True, (N,)), mean=(want_mean, (N, T, d)), cov=(want_cov, (N, T, d, d)), ess=(want_ess, (N, T)),
                       psi_mean=(want_psi_mean, (N, T, d + 1)), psi_var=(want_psi_var, (N, T, d + 1)), means=(want_means, (N, d, P)),
                       covs=(want_covs, (N, d * (d + 1) // 2, P)), weights=(want_weights, (N, P)), psi=(want_psi, (N, d + 1, P)))
        desc = _lib.RbDesc(P, int(n0), 1 if literal else 0, 1 if learn_v else 0, float(a))
        self._call("dlm_rb_batch", be, flags, md, pd, desc, pvb, pv_stride, pwb, pw_stride, yb, int(iteration), op, *out.values())
        return out

    def pf_forecast_learned(self, mat, params, cloud, var_w, var_v=None, *, family, var_kind, shapes=None, weights=None, ranks=(),
                            slot_offset=0, obs_param=None, iteration=0, seed=0, series_offset=0, flags=0, want_draws=False, want_mean=True,
                            want_cloud=True, want_var=True):
        """Posterior-predictive forecast from the cloud of a learning filter (dlm_pf_forecast_learned): `pf_forecast` with a diagonal state
        noise and an observation scale PER PARTICLE.  cloud [N][d][P]; var_w [N][d][P] and var_v [N][P] (None: every particle takes
        params' V) the particles' rows, read by var_kind: _lib.FC_VAR variances, _lib.FC_LOGVAR log-variances (`psi` of lw_filter and
        rb_filter), _lib.FC_IG_SCALE the InverseGamma scales of storvik_filter with shapes [d+1] or [N][d+1] (V's last), from which every
        particle draws its variances ONCE.  weights [N][P]: the cloud's weights (None: equal; given: the tuples are resampled once at
        entry).  mat describes the H forecast steps as for pf_forecast; a pure forecast -- nothing is observed: to fold in test-period
        observations, run the filter over them first.  params: V alone is read (without var_v).  ranks, slot_offset, obs_param as in
        pf_forecast.  Returns {"fmean" [N][H], "fquant" [N][H][len(ranks)], "draws" [N][H][P], "mean" [N][H][d] the mean of the cloud,
        "cloud" [N][d][P], "var_w" [N][d][P] and "var_v" [N][P] the variances the steps used, "status" [N]}; the optional ones are None
        when not wanted.  A series with a status bit has NaN from the failing step on."""
        if cloud is None or var_w is None:
            raise EngineError("the forecast from a learning filter needs its cloud and the particles' variance rows var_w")
        if len(cloud.shape) != 3:
            raise EngineError(f"cloud must be [N][d][P], got the shape {tuple(cloud.shape)}")
        N, P = int(cloud.shape[0]), int(cloud.shape[2])
        d, T, P = _pf_shape(mat, P, family)
        check_pf_forecast_learned_lds(d, P)
        rk = check_pf_ranks(ranks, P)
        if var_kind not in (_lib.FC_VAR, _lib.FC_LOGVAR, _lib.FC_IG_SCALE):
            raise EngineError(f"var_kind must be one of _lib.FC_* (0..2), got {var_kind!r}")
        if var_kind == _lib.FC_IG_SCALE and shapes is None:
            raise EngineError("FC_IG_SCALE needs shapes: the InverseGamma shapes of the d + 1 components")
        if var_v is not None and var_kind != _lib.FC_VAR and family in (_lib.OBS_NEGBIN, _lib.OBS_ZIP):
            raise EngineError("var_v of OBS_NEGBIN and OBS_ZIP is no variance (a log size, a logit): FC_VAR only")
        if family == _lib.OBS_STUDENTT and obs_param is None:
            raise EngineError("OBS_STUDENTT needs obs_param: the degrees of freedom (a scalar or one per series)")
        if not 0 <= int(slot_offset) <= _lib.PF_MAX_T - T:
            raise EngineError(f"slot_offset + the number of steps must stay within {_lib.PF_MAX_T} (the Philox counter's slot field), got {slot_offset} + {T}")
        be = self._backend(cloud)
        cb, wb, pwb, pvb = be.put(cloud), be.put(weights), be.put(var_w), be.put(var_v)
        for name, b, shape in (("cloud", cb, (N, d, P)), ("var_w", pwb, (N, d, P)), ("var_v", pvb, (N, P)), ("weights", wb, (N, P))):
            if b is not None and tuple(b.shape) != shape:
                raise EngineError(f"{name} must have the shape {shape}, got {tuple(b.shape)}")
        ob = None
        if obs_param is not None:
            ob = be.put(np.full(N, float(obs_param)) if np.ndim(obs_param) == 0 else obs_param)
            if tuple(ob.shape) != (N,):
                raise EngineError(f"obs_param must be a scalar or [N] = {(N,)}, got {tuple(ob.shape)}")
        sb, s_stride = None, 0
        if var_kind == _lib.FC_IG_SCALE:
            sh, s_stride = _strided(shapes, d + 1)
            sb = be.put(sh)
            if tuple(sb.shape) not in ((d + 1,), (N, d + 1)):
                raise EngineError(f"shapes must be [d+1] = {(d + 1,)} or [N][d+1], got {tuple(sb.shape)}")
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride and var_v is None:
            raise EngineError("the forecast from a learning filter takes a time-invariant V")
        out = _outputs(be, N, fmean=(True, (N, T)), fquant=(bool(rk), (N, T, len(rk))), draws=(want_draws, (N, T, P)),
                       mean=(want_mean, (N, T, d)), cloud=(want_cloud, (N, d, P)), var_w=(want_var, (N, d, P)), var_v=(want_var, (N, P)))
        desc = _lib.PfForecastLearnedDesc(int(family), P, int(var_kind), len(rk), int(slot_offset))
        rkc = (ctypes.c_int32 * len(rk))(*rk) if rk else None          # a host array whatever the backend: the call reads it before it returns
        self._call("dlm_pf_forecast_learned", be, flags, md, pd, desc, ob, rkc, cb, wb, pwb, pvb, sb, s_stride, int(iteration), op,
                   *out.values())
        return out

    def rb_state_draw(self, means, covs, *, slot, iteration=0, seed=0, series_offset=0, flags=0):
        """A state per particle from the Kalman moments rb_filter leaves (dlm_rb_state_draw): x_i = m_i + chol(C_i) z_i from means
        [N][d][P] and covs [N][d(d+1)/2][P] (the lower triangles by rows); the normals come from the Philox slot `slot` of the
        Rao-Blackwellised filter's stream, in blocks of their own (the number of steps filtered is the natural slot).  Returns {"cloud"
        [N][d][P], "status" [N]}; a series with a covariance that is not positive definite has DLM_ST_NOT_PD and NaN in its cloud."""
        if len(means.shape) != 3:
            raise EngineError(f"means must be [N][d][P], got the shape {tuple(means.shape)}")
        N, d, P = (int(s) for s in means.shape)
        check_pf_shape(d, 1, P)
        if tuple(covs.shape) != (N, d * (d + 1) // 2, P):
            raise EngineError(f"covs must be [N][d(d+1)/2][P] = {(N, d * (d + 1) // 2, P)}, got {tuple(covs.shape)}")
        if not 0 <= int(slot) <= _lib.PF_MAX_T + 1:
            raise EngineError(f"slot must satisfy 0 <= slot <= {_lib.PF_MAX_T + 1} (the Philox counter's slot field), got {slot}")
        be = self._backend(means)
        out = _outputs(be, N, cloud=(True, (N, d, P)))
        self._call("dlm_rb_state_draw", be, flags, d, N, P, be.put(means), be.put(covs), int(slot), int(iteration),
                   _options(be, flags, seed, series_offset), *out.values())
        return out

    def pg_sweep(self, mat, params, y, ref, *, family, n_particles, ancestor_sampling=True, obs_param=None, iteration=0, seed=0,
                 series_offset=0, flags=0, in_place=False, want_path_index=False, want_trace=False, want_step_weights=False,
                 workspace_cap=0):
        """One particle-Gibbs draw of the state path of N series (dlm_pg_batch): conditional SMC with P = n_particles particles, the last
        of which is the reference path ref [N][T+1][d] (dlm_ffbs_batch's convention: record 0 is the state before the first step, y[t]
        belongs to record t + 1), with ancestor sampling unless ancestor_sampling=False.  y [N][T] (NaN = missing), params and family as
        `particle_filter`.  in_place=True writes the new path over `ref` (which must then be a contiguous float64 array of the backend).
        Returns {"ll" [N], "path" [N][T+1][d], "stats" [N][d + 3] = [ssy | n | ss | T] of the drawn path (what `dinvgamma_step` takes),
        "path_index" [N][T+1] int32 (want_path_index), "clouds" [N][T+1][d][P] and "ancestors" [N][T][P] int32 (want_trace),
        "step_weights" [N][T][P] (want_step_weights), "status" [N]}; what was not wanted is None.  workspace_cap: the bytes of engine
        workspace one launch may take (0: _lib.PG_WORKSPACE_CAP); a larger batch runs as several launches, with the same results."""
        be = self._backend(y)
        d, T, P = _pf_shape(mat, n_particles, family)
        N, yb, ob = _pf_data(be, y, T, family, obs_param)
        if tuple(ref.shape) != (N, T + 1, d):
            raise EngineError(f"ref must be [N][T+1][d] = {(N, T + 1, d)}, got {tuple(ref.shape)}")
        rb = be.put(ref)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        if pd.v_tstride or pd.w_tstride:
            raise EngineError("particle Gibbs takes time-invariant V and W")
        out = _outputs(be, N, ll=(True, (N,)), path=rb if in_place else be.empty((N, T + 1, d)), stats=(True, (N, d + 3)),
                       path_index=(want_path_index, (N, T + 1), np.int32), clouds=(want_trace, (N, T + 1, d, P)),
                       ancestors=(want_trace, (N, T, P), np.int32), step_weights=(want_step_weights, (N, T, P)))
        desc = _lib.PgDesc(int(family), P, 1 if ancestor_sampling else 0, int(workspace_cap))
        self._call("dlm_pg_batch", be, flags, md, pd, desc, ob, yb, rb, int(iteration), op, *out.values())
        return out

    def simulate(self, mat, params, N, *, seed=0, series_offset=0, device=False, want_x=True):
        """Dlm.simulateRegular over the model's time grid for N series (dlm_simulate_batch): (x [N][T+1][d], y [N][T][p])."""
        be = _Device(self.device) if device else _Host()
        d, p, T = mat.d, mat.p, mat.T
        md, pd, op, keep = self.prepare(mat, params, N, be, 0, seed, series_offset)
        out = _outputs(be, N, x=(want_x, (N, T + 1, d)), y=(True, (N, T, p)))
        self._call("dlm_simulate_batch", be, 0, md, pd, op, *out.values())
        return out

    def smooth(self, mat, params, filt, *, flags=0):
        be = self._backend(filt)
        N = int(filt.shape[0]); d, T = mat.d, mat.T
        fb = be.put(filt)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags)
        out = _outputs(be, N, smooth=(True, (N, T + 1, d + d * d)))
        self._call("dlm_smooth_batch", be, flags, md, pd, fb, op, *out.values())
        return out

    def filter_smooth(self, mat, params, y, *, flags=0, out=None, want_filt=True):
        """Fused filter + smoother.  want_filt=False keeps the filtered records inside the engine (packed on the
        structured fast path) and returns only the smoothed moments.  flags & OPT_PACKED_SYM: both outputs are packed
        records [mean | lower triangle by rows] (dlm_packed_record_doubles(d) doubles; unpack_records expands them)."""
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        recw = self.lib.dlm_packed_record_doubles(d) if flags & _lib.OPT_PACKED_SYM else d + d * d
        yb = be.put(y).reshape(N, T, p)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags)
        filt = (out["filt"] if out else be.empty((N, T + 1, recw))) if want_filt else None
        res = _outputs(be, N, out["status"] if out else None, filt=filt, smooth=out["smooth"] if out else be.empty((N, T + 1, recw)))
        self._call("dlm_filter_smooth_batch", be, flags, md, pd, yb, op, *res.values())
        return res

    def unpack_records(self, d, packed):
        """Packed records [..., dlm_packed_record_doubles(d)] -> dense [..., d + d*d] (dlm_unpack_records)."""
        be = self._backend(packed)
        pb = be.put(packed)
        count = int(np.prod(pb.shape[:-1]))
        dense = be.empty(tuple(pb.shape[:-1]) + (d + d * d,))
        self._call("dlm_unpack_records", be, 0, int(d), count, pb, _options(be), dense)
        return dense

    def last_timing(self):
        """(forward_ms, backward_ms) of the last fused call, from HIP events on the engine stream."""
        ms = (ctypes.c_double * 2)()
        self._check(self.lib.dlm_last_timing(self.h, ctypes.byref(ms)))
        return float(ms[0]), float(ms[1])

    def last_counters(self):
        """(forward steady steps, backward steady steps, series on the shared-covariance path, series on their own
        recursion) of the last call made with DLM_OPT_COUNT_STEPS."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self.lib.dlm_last_counters(self.h, ctypes.byref(c)))
        return tuple(int(v) for v in c)

    def last_table_reuse(self):
        """What the last filter_smooth call did about the shared RTS tables: _lib.TABLES_NONE / TABLES_BUILT / TABLES_REUSED /
        TABLES_SKIPPED (dlm_last_table_reuse)."""
        v = ctypes.c_int32(0)
        self._check(self.lib.dlm_last_table_reuse(self.h, ctypes.byref(v)))
        return int(v.value)

    def ffbs(self, mat, params, y, *, z=None, seed=0, series_offset=0, flags=0, want_theta=True,
             want_cond=False, want_stats=True, filt=None, want_filt=True):
        """FFBS (filt=None) or backward sampling from existing filter records (filt given).  want_filt=False: the forward
        pass's records are not wanted (dlm_ffbs_batch with filt_ws = NULL)."""
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        rec = d + d * d
        yb = be.put(y).reshape(N, T, p)
        zb, fb = be.put(z), be.put(filt)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        L = self.lib.dlm_stats_len(d, p, flags & ~_lib.OPT_FFBS_SIMSMOOTH)
        out = _outputs(be, N, theta=(want_theta, (N, T + 1, d)), cond=(want_cond, (N, T + 1, rec)), stats=(want_stats, (N, L)),
                       filt=(want_filt, (N, T + 1, rec)) if filt is None else fb)
        ws, rest = out["filt"], (out["theta"], out["cond"], out["stats"], out["status"])
        if filt is None:
            self._call("dlm_ffbs_batch", be, flags, md, pd, yb, zb, op, ws, *rest)
        else:
            self._call("dlm_backward_sample_batch", be, flags, md, pd, yb, ws, zb, op, *rest)
        return out

    def svd_filter(self, mat, params, y, *, flags=0):
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        yb = be.put(y).reshape(N, T, p)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags)
        out = _outputs(be, N, svd=(True, (N, T + 1, 2 * d + d * d)))
        self._call("dlm_svd_filter_batch", be, flags, md, pd, yb, op, *out.values())
        return out

    def svd_ffbs(self, mat, params, y, *, z=None, seed=0, series_offset=0, flags=0, want_stats=True):
        be = self._backend(y)
        N = int(y.shape[0]); d, p, T = mat.d, mat.p, mat.T
        yb = be.put(y).reshape(N, T, p)
        zb = be.put(z)
        md, pd, op, keep = self.prepare(mat, params, N, be, flags, seed, series_offset)
        out = _outputs(be, N, svd=(True, (N, T + 1, 2 * d + d * d)), theta=(True, (N, T + 1, d)),
                       stats=(want_stats, (N, self.lib.dlm_stats_len(d, p, flags))))
        self._call("dlm_svd_ffbs_batch", be, flags, md, pd, yb, zb, op, *out.values())
        return out

    def stats_pool(self, stats):
        be = self._backend(stats)
        N, L = int(stats.shape[0]), int(stats.shape[1])
        sb = be.put(stats)
        pooled = be.empty((L,))
        self._call("dlm_stats_pool", be, 0, sb, N, L, pooled, _options(be))
        return pooled

    # -- RCCL ----------------------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
        rc = self.lib.dlm_comm_unique_id(buf)
        if rc != 0:
            raise EngineError(f"dlm_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init_rank(self, nranks: int, rank: int, uid: bytes):
        self._check(self.lib.dlm_comm_init_rank(self.h, nranks, rank, ctypes.create_string_buffer(uid, _lib.COMM_ID_BYTES)))

    def allreduce_stats(self, stats_dev):
        """In-place RCCL sum of a device fp64 tensor."""
        self._check(self.lib.dlm_gibbs_suffstats_allreduce(self.h, ctypes.c_void_p(stats_dev.data_ptr()),
                                                           stats_dev.numel()))
        return stats_dev
