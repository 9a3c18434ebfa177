"""A guarded, fused Adam step for the trainers (--fused-optim): `fused_adam_numpy`, the specification, and `FusedAdam`, a
torch.optim.Optimizer over liblav_amd's lav_optim_adam_step (csrc/optim.hip, include/lav_amd.h) with the specification as its CPU path.

One step reads every gradient once for two statistics - how many elements are NaN or +-Inf, and the float64 sum of the squares of the
others - and decides: with a single element that is not finite the step is SKIPPED (nothing is stored but a counter), otherwise it is
APPLIED, clipped to `max_norm` by clip_grad_norm_'s factor when one is set:

    clip         = float32(min(1, max_norm / (sqrt(sumsq) + 1e-6)))                 (1 without a limit)
    per tensor, float64:  step += 1;  beta1_power *= beta1;  beta2_power *= beta2
                 step_size    = float32(lr / (1 - beta1_power))
                 inv_sqrt_bc2 = float32(1 / sqrt(1 - beta2_power))
    per element, float32, every operation rounded on its own (the constants beta and 1 - beta are float64 values rounded once:
    float32(1) - float32(0.999) is 1.3e-5 away from 0.001, float32(1 - 0.999) is not):
                 g' = g * clip
                 m  = beta1 * m + (1 - beta1) * g'
                 v  = beta2 * v + ((1 - beta2) * g') * g'
                 p  = p - step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps))

Running products stand where torch has beta ** step, so that host and device agree bit for bit; steps are counted per tensor, as torch
counts them (a parameter without a gradient is left out of that step and keeps its own count).  The words are laid out as the C ABI
lays them out (TENSOR_DTYPE ... GLOBAL_DTYPE = lav_optim_tensor ... lav_optim_global).

With an `ema_decay` (0 < decay < 1; FusedAdam(ema_decay=), the trainers' --ema) an applied step also moves a shadow e of every tensor it
updates towards the parameter it has just computed (lav_optim_adam_ema_step: inside the update launch, which still holds p):

    per tensor, float64, k = its step count after this step:  d_k = min(ema_decay, (1 + k) / (10 + k));  omd = float32(1 - d_k)
    per element, float32, every operation rounded on its own:  e = e + omd * (p - e)

The warm-up keeps the first steps from being dominated by where the shadow started; a skipped step leaves e alone, as it leaves p.

The per-tensor view (FusedAdam.tensor_stats(), the trainers' --tensor-stats N; lav_optim_tensor_stats) says WHERE a run goes wrong:
`tensor_stats_numpy` is its specification, one TENSOR_ROW_DTYPE row per tensor of the step and one WATCH_ROW_DTYPE row per watched
buffer.  The histogram of a gradient is a pure function of the float32 bit pattern, exact and free of any order: with e the biased
exponent field, a finite element counts in bin clamp(e - 86, 0, 63) - bin 0 holds zeros, denormals and everything below 2^-40, bin k
(1 .. 62) holds [2^(k-41), 2^(k-40)), bin 63 holds finite values >= 2^22; elements that are not finite count in g_nonfinite alone.
This differs from the reference's wandb.watch (lav/utils/logger.py:32) on purpose: wandb draws 64 LINEAR bins between the minimum and the
maximum, which needs two passes over the data and resolves nothing across a gradient's dynamic range - one outlier puts every other
element into bin 0.  `blame_numpy` is the specification of lav_optim_blame: the ring that names the tensors of a skipped step."""
from __future__ import annotations

import math

import numpy as np
import torch
from torch.optim import Optimizer

TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("numel", "<i8"), ("lr", "<f8"), ("beta1", "<f8"),
                         ("beta2", "<f8"), ("eps", "<f8"), ("state", "<i4"), ("chunk0", "<i4")])
WATCH_DTYPE = np.dtype([("data", "<u8"), ("numel", "<i8"), ("chunk0", "<i4"), ("reserved", "<i4")])
STATE_DTYPE = np.dtype([("step", "<i8"), ("beta1_power", "<f8"), ("beta2_power", "<f8"), ("step_size", "<f4"), ("inv_sqrt_bc2", "<f4")])
GLOBAL_DTYPE = np.dtype([("applied", "<i8"), ("skipped", "<i8"), ("nonfinite", "<i8"), ("sumsq", "<f8"), ("clip", "<f4"), ("apply", "<i4"),
                         ("watch_nonfinite", "<i8")])
assert (TENSOR_DTYPE.itemsize, WATCH_DTYPE.itemsize, STATE_DTYPE.itemsize, GLOBAL_DTYPE.itemsize) == (80, 24, 32, 48)
HIST_BINS, BLAME_RING, BLAME_PER_STEP = 64, 16, 4      # LAV_OPTIM_HIST_BINS, LAV_OPTIM_BLAME_RING, LAV_OPTIM_BLAME_PER_STEP
TENSOR_ROW_DTYPE = np.dtype([("g_sumsq", "<f8"), ("p_sumsq", "<f8"), ("u_sumsq", "<f8"), ("g_nonfinite", "<i8"), ("g_zeros", "<i8"),
                             ("p_nonfinite", "<i8"), ("g_maxabs", "<f4"), ("p_maxabs", "<f4"), ("u_maxabs", "<f4"), ("reserved", "<i4"),
                             ("hist", "<i8", (HIST_BINS,))])
WATCH_ROW_DTYPE = np.dtype([("nonfinite", "<i8"), ("maxabs", "<f4"), ("reserved", "<i4")])
BLAME_RECORD_DTYPE = np.dtype([("step", "<i8"), ("nonfinite", "<i8"), ("index", "<i4"), ("reserved", "<i4")])
BLAME_DTYPE = np.dtype([("written", "<i8", (2,)), ("ring", BLAME_RECORD_DTYPE, (2, BLAME_RING))])      # [0] tensors, [1] watched buffers
assert (TENSOR_ROW_DTYPE.itemsize, WATCH_ROW_DTYPE.itemsize, BLAME_RECORD_DTYPE.itemsize, BLAME_DTYPE.itemsize) == (576, 16, 24, 784)


def new_state(n):
    """The words of n tensors before their first step: step 0, both powers 1."""
    st = np.zeros(n, STATE_DTYPE)
    st["beta1_power"] = 1.0
    st["beta2_power"] = 1.0
    return st


def chunk_length():
    """Elements per workgroup of the device kernels (lav_optim_chunk)."""
    from .. import _lib
    return int(_lib.load().lav_optim_chunk())


def fill_chunks(rows, chunk):
    """rows["chunk0"] from rows["numel"]; returns the chunks in all."""
    n = (rows["numel"] + chunk - 1) // chunk
    if len(rows) and n.min() < 1:
        raise ValueError("a row of the table has no element")
    total = int(n.sum())
    if total > 0x7FFFFFFF:
        raise ValueError(f"{total} chunks")
    rows["chunk0"] = np.cumsum(n) - n
    return total


def fused_adam_numpy(tensors, state, glob, max_norm=None, watch=(), sumsq=None, ema_decay=None):
    """The specification of one step (see the module's text).  tensors: one dict per tensor of the step with p, g, m, v (1-D float32
    arrays; p, m, v are updated in place), lr, beta1, beta2, eps and `state`, its index in `state` (a STATE_DTYPE array, updated in
    place); glob: a GLOBAL_DTYPE array of one element; watch: float32 arrays that are only scanned; sumsq: taken in place of this
    function's own float64 sum of squares (whose order is NumPy's) - for a comparison in which the clip factor is in play.
    ema_decay: a row that carries `e` (a float32 array like p) has it moved towards the new p, in place."""
    if ema_decay is not None and not 0.0 < ema_decay < 1.0:
        raise ValueError(f"fused_adam_numpy: ema_decay {ema_decay} (0 < decay < 1, or None)")
    g_all = [np.asarray(t["g"]) for t in tensors]
    if any(g.dtype != np.float32 for g in g_all):
        raise TypeError("fused_adam_numpy: float32 gradients")
    bad = 0
    own = 0.0
    for g in g_all:
        fin = np.isfinite(g)
        bad += int(g.size - np.count_nonzero(fin))
        own += float(np.sum(np.square(g[fin].astype(np.float64)), dtype=np.float64))
    total = np.float64(own if sumsq is None else sumsq)
    clip = np.float32(1)
    if max_norm is not None and max_norm > 0:
        clip = np.float32(min(np.float64(1), np.float64(max_norm) / (np.sqrt(total) + np.float64(1e-6))))
    w = glob[0] if getattr(glob, "ndim", 0) else glob
    w["nonfinite"], w["sumsq"], w["clip"], w["apply"] = bad, total, clip, int(bad == 0)
    w["watch_nonfinite"] = sum(int(b.size - np.count_nonzero(np.isfinite(b))) for b in (np.asarray(b) for b in watch))
    if bad:
        w["skipped"] += 1
        return
    w["applied"] += 1
    one = np.float64(1)
    with np.errstate(all="ignore"):
        for t, g in zip(tensors, g_all):
            st = state[t["state"]:t["state"] + 1]
            b1p = st["beta1_power"][0] * np.float64(t["beta1"])
            b2p = st["beta2_power"][0] * np.float64(t["beta2"])
            st["step"] += 1
            st["beta1_power"], st["beta2_power"] = b1p, b2p
            step_size = np.float32(np.float64(t["lr"]) / (one - b1p))
            inv = np.float32(one / np.sqrt(one - b2p))
            st["step_size"], st["inv_sqrt_bc2"] = step_size, inv
            beta1, beta2, eps = np.float32(t["beta1"]), np.float32(t["beta2"]), np.float32(t["eps"])
            om1, om2 = np.float32(one - np.float64(t["beta1"])), np.float32(one - np.float64(t["beta2"]))
            p, m, v = t["p"], t["m"], t["v"]
            gs = g * clip
            m[...] = beta1 * m + om1 * gs
            v[...] = beta2 * v + (om2 * gs) * gs
            p[...] = p - step_size * (m / (np.sqrt(v) * inv + eps))
            e = t.get("e") if ema_decay is not None else None
            if e is not None:
                omd = np.float32(one - ema_decay_at(ema_decay, st["step"][0]))
                e[...] = e + omd * (p - e)


def ema_decay_at(ema_decay, k):
    """d_k, float64: the decay of the step that brings a tensor's count to k >= 1."""
    k = np.float64(k)
    return min(np.float64(ema_decay), (np.float64(1) + k) / (np.float64(10) + k))


def _finite_view(x):
    """(finite elements as float32, their count of the others, the largest finite |x| as a float32): maxima on the values, which for
    finite floats order as the bit patterns of |x| do."""
    x = np.asarray(x, np.float32).reshape(-1)
    fin = x[np.isfinite(x)]
    return fin, int(x.size - fin.size), (np.float32(np.abs(fin).max()) if fin.size else np.float32(0))


def _sumsq(fin):
    return float(np.sum(np.square(fin.astype(np.float64)), dtype=np.float64))


def update_term_numpy(t, st):
    """u = step_size * (m / (sqrt(v) * inv_sqrt_bc2 + eps)) of one row in float32, every operation rounded on its own, from the tensor's
    stored words `st` and m, v as they stand: what the last applied step subtracted from p.  A tensor at step 0 gives 0."""
    m, v = np.asarray(t["m"], np.float32).reshape(-1), np.asarray(t["v"], np.float32).reshape(-1)
    if int(st["step"]) <= 0:
        return np.zeros_like(m)
    with np.errstate(all="ignore"):
        return np.float32(st["step_size"]) * (m / (np.sqrt(v) * np.float32(st["inv_sqrt_bc2"]) + np.float32(t["eps"])))


def tensor_stats_numpy(tensors, state, watch=()):
    """The specification of lav_optim_tensor_stats (the module's text): tensors and state as fused_adam_numpy takes them (nothing is
    changed), watch: float32 arrays.  Returns (TENSOR_ROW_DTYPE rows, WATCH_ROW_DTYPE rows)."""
    rows, wrows = np.zeros(len(tensors), TENSOR_ROW_DTYPE), np.zeros(len(watch), WATCH_ROW_DTYPE)
    for r, t in enumerate(tensors):
        g, bad, mx = _finite_view(t["g"])
        bits = g.view(np.uint32) & np.uint32(0x7FFFFFFF)
        bins = np.clip((bits >> np.uint32(23)).astype(np.int64) - 86, 0, HIST_BINS - 1)
        rows[r]["g_nonfinite"], rows[r]["g_zeros"], rows[r]["g_sumsq"], rows[r]["g_maxabs"] = bad, int(np.count_nonzero(bits == 0)), _sumsq(g), mx
        rows[r]["hist"] = np.bincount(bins, minlength=HIST_BINS)
        p, bad, mx = _finite_view(t["p"])
        rows[r]["p_nonfinite"], rows[r]["p_sumsq"], rows[r]["p_maxabs"] = bad, _sumsq(p), mx
        u, _, mx = _finite_view(update_term_numpy(t, state[t["state"]]))
        rows[r]["u_sumsq"], rows[r]["u_maxabs"] = _sumsq(u), mx
    for r, b in enumerate(watch):
        _, wrows[r]["nonfinite"], wrows[r]["maxabs"] = _finite_view(b)
    return rows, wrows


def blame_numpy(tensors, glob, blame, watch=()):
    """The specification of lav_optim_blame, called behind fused_adam_numpy with the same tensors, words and watched arrays: when that
    step was skipped (glob apply == 0) the first BLAME_PER_STEP tensors, in table order, whose gradient holds elements that are not
    finite are appended to ring 0 of `blame` (a BLAME_DTYPE array of one element, changed in place) as (step = applied + skipped, the
    count, the row's `state`), and the first BLAME_PER_STEP watched arrays with such elements to ring 1, index = their position in
    `watch`.  Record k of a ring lies in slot k % BLAME_RING; written counts the records ever appended.  An applied step writes nothing."""
    w = glob[0] if getattr(glob, "ndim", 0) else glob
    if int(w["apply"]):
        return
    b = blame[0] if getattr(blame, "ndim", 0) else blame
    step = int(w["applied"]) + int(w["skipped"])
    for k, rows in enumerate(([(t["state"], t["g"]) for t in tensors], list(enumerate(watch)))):
        found = 0
        for index, x in rows:
            bad = _finite_view(x)[1]
            if bad and found < BLAME_PER_STEP:
                b["ring"][k][int(b["written"][k]) % BLAME_RING] = (step, bad, index, 0)
                b["written"][k] += 1
                found += 1


def blame_records(blame, names=None):
    """The records a BLAME_DTYPE block still holds, oldest first: ([tensors], [watched buffers]) of dicts step, index, nonfinite, ordinal
    (the record's number since the block was zeroed) and, with names = (parameter names, buffer names), name."""
    b = blame[0] if getattr(blame, "ndim", 0) else blame
    out = []
    for k in range(2):
        written = int(b["written"][k])
        recs = []
        for o in range(max(0, written - BLAME_RING), written):
            rec = b["ring"][k][o % BLAME_RING]
            d = dict(step=int(rec["step"]), index=int(rec["index"]), nonfinite=int(rec["nonfinite"]), ordinal=o)
            if names is not None:
                d["name"] = names[k][d["index"]]
            recs.append(d)
        out.append(recs)
    return tuple(out)


_ADAM_DEFAULTS = dict(weight_decay=0.0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                      decoupled_weight_decay=False)      # torch.optim.Adam's other group keys: a state_dict moves between the two classes


class FusedAdam(Optimizer):
    """Adam (torch.optim.Adam's defaults, no weight decay, no amsgrad) whose step is the module's specification: on cuda parameters
    three launches of liblav_amd over all of them (lav_optim_adam_step), on CPU parameters fused_adam_numpy.  max_grad_norm: clip the
    global gradient norm (clip_grad_norm_'s factor) inside the same step; watch: float32 buffers scanned for values that are not finite
    by the same launch (BatchNorm's running statistics).  step() never waits for the device; health() does, for six words.
    state_dict() has torch.optim.Adam's layout (step, exp_avg, exp_avg_sq per parameter) plus beta1_power / beta2_power, Python floats
    (float64: load_state_dict casts tensors to the parameter's dtype, and leaves numbers alone); a torch.optim.Adam state loads into it
    (a missing power is beta ** step) and its state loads into torch.optim.Adam.
    ema_decay: keep state[p]["ema"], an exponential moving average of p (the module's text), beside exp_avg: a clone of p taken before
    the parameter's first update here - also where a loaded state has none (a torch.optim.Adam state, a run started without it; the
    warm-up then goes on from the loaded step count).  It travels in state_dict(); torch.optim.Adam ignores the key and keeps it.
    names: (one unique name per parameter in group order, one per watched buffer) - the trainers' --tensor-stats.  With names every
    step() is followed by lav_optim_blame on the same stream (blame(): which tensors made a step skip), and tensor_stats() may be called
    behind a step for the per-tensor view of it.  Without names neither is launched and nothing is allocated for them."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False, max_grad_norm=None,
                 watch=(), ema_decay=None, names=None):
        if not 0.0 <= lr or not 0.0 <= eps or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdam: lr {lr}, eps {eps}, betas {betas}")
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdam: max_grad_norm {max_grad_norm} (a positive norm, or None)")
        if ema_decay is not None and not 0.0 < ema_decay < 1.0:
            raise ValueError(f"FusedAdam: ema_decay {ema_decay} (0 < decay < 1, or None)")
        defaults = dict(_ADAM_DEFAULTS, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.watch = tuple(watch)
        for b in self.watch:
            if not (isinstance(b, torch.Tensor) and b.dtype == torch.float32 and b.layout == torch.strided and b.is_contiguous()):
                raise TypeError("FusedAdam: watch holds dense float32 tensors")
        self._check()
        self.names = None
        if names is not None:
            self.names = (tuple(names[0]), tuple(names[1]))
            if len(self.names[0]) != len(self._params()) or len(self.names[1]) != len(self.watch) or \
                    len(set(self.names[0] + self.names[1])) != len(self.names[0]) + len(self.names[1]):
                raise ValueError("FusedAdam: names holds one unique name per parameter and one per watched buffer")
        self._blame = self._rows_out = self._last = None        # names alone: the blame block; the rows' device buffer; the CPU step's arrays
        self._words = None          # STATE_DTYPE rows, one per parameter in group order: a uint8 tensor on the parameters' device
        self._global = None         # GLOBAL_DTYPE, there too
        self._key = self._table = self._watch_table = self._shadow_table = self._host = None
        self._counts = (0, 0, 0, 0)

    # ------------------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _check(self):
        for group in self.param_groups:
            for k in ("amsgrad", "maximize"):
                if group.get(k):
                    raise ValueError(f"FusedAdam: {k} is not supported")
            if group.get("weight_decay"):
                raise ValueError(f"FusedAdam: weight_decay {group['weight_decay']} is not supported (0 only)")
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(f"FusedAdam: float32 parameters only, got {p.dtype}")
                if p.layout != torch.strided or not p.is_contiguous():
                    raise ValueError("FusedAdam: dense (contiguous, strided) parameters only")
        devs = {p.device for p in self._params()}
        if len(devs) > 1:
            raise ValueError(f"FusedAdam: parameters on one device only, got {sorted(map(str, devs))}")
        return next(iter(devs))

    def _ensure_words(self, device):
        n = len(self._params())
        if self._words is not None and self._words.numel() == n * STATE_DTYPE.itemsize and self._words.device == device:
            return
        self._words = torch.from_numpy(self._state_rows().view(np.uint8)).to(device)
        if self._global is None or self._global.device != device:
            self._global = torch.zeros(GLOBAL_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self._key = None

    def _state_rows(self):
        """STATE_DTYPE rows from self.state (a parameter without state: step 0)."""
        params = self._params()
        rows = new_state(len(params))
        i = 0
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    step = int(round(float(st["step"])))
                    b1p = float(st["beta1_power"]) if "beta1_power" in st else float(beta1) ** step
                    b2p = float(st["beta2_power"]) if "beta2_power" in st else float(beta2) ** step
                    rows[i] = (step, b1p, b2p, 0.0, 0.0)
                    if step > 0:
                        rows[i]["step_size"] = np.float32(np.float64(group["lr"]) / (np.float64(1) - np.float64(b1p)))
                        rows[i]["inv_sqrt_bc2"] = np.float32(np.float64(1) / np.sqrt(np.float64(1) - np.float64(b2p)))
                i += 1
        return rows

    def _rows_host(self):
        return self._words.cpu().numpy().view(STATE_DTYPE)

    def _pull(self):
        """The device's words into self.state (one device -> host read)."""
        if self._words is None:
            return
        rows = self._rows_host()
        for i, p in enumerate(self._params()):
            st = self.state.get(p)
            if st:
                st["step"] = torch.tensor(float(rows[i]["step"]), dtype=torch.float32)
                st["beta1_power"], st["beta2_power"] = float(rows[i]["beta1_power"]), float(rows[i]["beta2_power"])

    def state_dict(self):
        self._pull()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        device = self._check()
        self._words = None
        self._ensure_words(device)

    def add_param_group(self, group):
        super().add_param_group(group)
        if getattr(self, "_words", None) is not None:
            self._pull()
            self._words = None

    def health(self):
        """The global words: applied / skipped steps of this object, and of the last step `nonfinite` gradient elements, `sumsq` and
        `grad_norm` = sqrt(sumsq) of the finite ones, `clip`, `apply`, `watch_nonfinite`.  One small device -> host read."""
        if self._global is None:
            w = np.zeros(1, GLOBAL_DTYPE)[0]
        else:
            w = self._global.cpu().numpy().view(GLOBAL_DTYPE)[0]
        out = {k: (float(w[k]) if k in ("sumsq", "clip") else int(w[k])) for k in GLOBAL_DTYPE.names}
        out["grad_norm"] = math.sqrt(out["sumsq"])
        return out

    def blame(self):
        """Read together with health() (one more small device -> host read): the records the blame block still holds, oldest first, as
        ([tensors], [watched buffers]) of dicts name, index, nonfinite, step (the ordinal applied + skipped of the skipped step, as
        health() counts them) and ordinal (the record's number: a gap to the last one seen says how many the ring lost)."""
        if self.names is None:
            raise RuntimeError("FusedAdam.blame: an optimiser without names records none")
        if self._blame is None:
            return [], []
        return blame_records(self._blame.cpu().numpy().view(BLAME_DTYPE), (self.names[0], self._watch_names()))

    def watched_nonfinite(self):
        """The watched buffers that hold values that are not finite, as blame()'s records (without a step): a look at each of them, for
        the message of a run that ends."""
        out = []
        for name, b in zip(self.names[1], self.watch):
            bad = int(b.numel() - int(torch.isfinite(b).sum()))
            if bad:
                out.append(dict(name=name, nonfinite=bad, global_it=None))
        return out

    def _watch_names(self):
        return [name for name, b in zip(self.names[1], self.watch) if b.numel() > 0]

    def tensor_stats(self):
        """The per-tensor view of the step that has just run (its gradients must still be alive): on cuda parameters two launches over
        the step's own tables (lav_optim_tensor_stats) and a non-blocking copy of the rows and the global words into a pinned slot of
        their own - nothing waits; on CPU parameters tensor_stats_numpy.  Returns a PendingTensorStats; its result() waits for the copy."""
        if self.names is None:
            raise RuntimeError("FusedAdam.tensor_stats: an optimiser without names")
        if self._words is None or (self._key is None and self._last is None):
            raise RuntimeError("FusedAdam.tensor_stats: behind a step()")
        device = self._words.device
        wnames = self._watch_names()
        if device.type != "cuda":
            tensors, watch = self._last
            rows, wrows = tensor_stats_numpy(tensors, self._words.numpy().view(STATE_DTYPE), watch)
            names = [self.names[0][t["state"]] for t in tensors]
            return PendingTensorStats(names, [t["p"].size for t in tensors], wnames, rows, wrows, self._global.numpy().view(GLOBAL_DTYPE)[0].copy())
        from .. import ops
        n, chunks, nw, wchunks = self._counts
        sizes = (n * TENSOR_ROW_DTYPE.itemsize, nw * WATCH_ROW_DTYPE.itemsize, GLOBAL_DTYPE.itemsize)
        if self._rows_out is None or self._rows_out.numel() != sum(sizes) or self._rows_out.device != device:
            self._rows_out = torch.zeros(sum(sizes), dtype=torch.uint8, device=device)
        out = self._rows_out
        ops.optim_tensor_stats(self._table, n, chunks, self._watch_table, nw, wchunks, self._words, out[:sizes[0]], out[sizes[0]:sizes[0] + sizes[1]])
        out[sizes[0] + sizes[1]:].copy_(self._global)
        host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        key = self._key[0]
        return PendingTensorStats([self.names[0][row[9]] for row in key], [row[4] for row in key], wnames, host, sizes, None, done)

    # ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        device = self._check()
        self._ensure_words(device)
        used, grads, key, shadows, i = [], [], [], [], 0
        for group in self.param_groups:
            lr, (beta1, beta2), eps = float(group["lr"]), group["betas"], float(group["eps"])
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    if g.is_sparse or g.dtype != torch.float32 or g.device != p.device:
                        raise ValueError("FusedAdam: dense float32 gradients on the parameter's device only")
                    if not g.is_contiguous():
                        g = g.contiguous()
                    st = self.state[p]
                    if "exp_avg" not in st:
                        st.setdefault("step", torch.tensor(0.0, dtype=torch.float32))
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    m, v = st["exp_avg"], st["exp_avg_sq"]
                    if self.ema_decay is not None:
                        e = st.get("ema")
                        if e is None:           # before the update: the first step here, or a loaded state without a shadow
                            e = st["ema"] = p.detach().clone(memory_format=torch.contiguous_format)
                        shadows.append(e)       # (checked where a table is built from them: the walk stays cheap)
                    used.append(p)
                    grads.append(g)         # (alive until the launches are enqueued)
                    key.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, float(beta1), float(beta2), eps, i))
                i += 1
        key = [row for row in key if row[4] > 0]
        wkey = [(b.data_ptr(), b.numel()) for b in self.watch if b.numel() > 0]
        shadows = [e for e in shadows if e.numel() > 0]
        if device.type == "cuda":
            self._step_device(device, key, wkey, shadows)
        else:
            self._step_host(used, grads, key)
        if used:    # a write through a raw pointer moves no version counter, and caches are keyed on it (lav_amd.rgb)
            torch.autograd.graph.increment_version(used)
        return loss

    def _step_host(self, used, grads, key):
        rows = self._words.numpy().view(STATE_DTYPE)
        glob = self._global.numpy().view(GLOBAL_DTYPE)
        tensors = []
        for p, g in zip(used, grads):
            if p.numel() == 0:
                continue
            st = self.state[p]
            _, _, _, _, _, lr, beta1, beta2, eps, i = key[len(tensors)]
            tensors.append(dict(p=p.detach().view(-1).numpy(), g=g.detach().view(-1).numpy(), m=st["exp_avg"].view(-1).numpy(),
                                v=st["exp_avg_sq"].view(-1).numpy(), lr=lr, beta1=beta1, beta2=beta2, eps=eps, state=i))
            if self.ema_decay is not None:
                self._check_shadows([p], [st["ema"]])
                tensors[-1]["e"] = st["ema"].view(-1).numpy()
        watch = [b.detach().view(-1).numpy() for b in self.watch if b.numel() > 0]
        fused_adam_numpy(tensors, rows, glob, self.max_grad_norm, watch, ema_decay=self.ema_decay)
        if self.names is not None:
            if self._blame is None:
                self._blame = torch.zeros(BLAME_DTYPE.itemsize, dtype=torch.uint8)
            blame_numpy(tensors, glob, self._blame.numpy().view(BLAME_DTYPE), watch)
            self._last = (tensors, watch)

    def _check_shadows(self, used, shadows):
        for p, e in zip(used, shadows):
            if e.dtype != torch.float32 or e.device != p.device or e.shape != p.shape or not e.is_contiguous():
                raise ValueError("FusedAdam: state['ema'] must be a dense float32 tensor of the parameter's shape, on its device")

    def _step_device(self, device, key, wkey, shadows=()):
        from .. import ops
        shadows = [e.data_ptr() for e in shadows]
        full = (tuple(key), tuple(wkey), tuple(shadows))
        if full != self._key:
            # a fresh pinned buffer and a fresh device table per change: the copy is ordered on the stream behind the launches that
            # read the table it replaces, and a source is never rewritten
            if shadows:
                by_index = self._params()
                self._check_shadows([by_index[row[9]] for row in key], [self.state[by_index[row[9]]]["ema"] for row in key])
            chunk = chunk_length()
            table = np.zeros(len(key), TENSOR_DTYPE)
            for r, row in enumerate(key):
                table[r] = row + (0,)
            watch = np.zeros(len(wkey), WATCH_DTYPE)
            for r, (ptr, n) in enumerate(wkey):
                watch[r] = (ptr, n, 0, 0)
            chunks, wchunks = fill_chunks(table, chunk), fill_chunks(watch, chunk)
            ptrs = np.asarray(shadows, "<u8")       # (the EMA entry's pointer array, row-parallel to the table; 8-byte aligned behind 80 / 24)
            blob = np.concatenate([table.view(np.uint8), watch.view(np.uint8), ptrs.view(np.uint8), np.zeros(16, np.uint8)])
            self._host = torch.from_numpy(blob).pin_memory()
            dev = self._host.to(device, non_blocking=True)
            self._table, self._watch_table = dev[:table.nbytes], dev[table.nbytes:table.nbytes + watch.nbytes]
            self._shadow_table = dev[table.nbytes + watch.nbytes:table.nbytes + watch.nbytes + ptrs.nbytes]
            self._counts = (len(key), chunks, len(wkey), wchunks)
            self._key = full
        n, chunks, nw, wchunks = self._counts
        if self.ema_decay is not None:
            ops.optim_adam_ema_step(self._table, n, chunks, self._watch_table, nw, wchunks, self._words, self._global, self._shadow_table,
                                    self.ema_decay, self.max_grad_norm)
        else:
            ops.optim_adam_step(self._table, n, chunks, self._watch_table, nw, wchunks, self._words, self._global, self.max_grad_norm)
        if self.names is not None:
            if self._blame is None or self._blame.device != device:
                self._blame = torch.zeros(BLAME_DTYPE.itemsize, dtype=torch.uint8, device=device)
            ops.optim_blame(self._table, n, chunks, self._watch_table, nw, wchunks, self._global, self._blame)


class PendingTensorStats:
    """What FusedAdam.tensor_stats() returns: the rows of one step, possibly still on their way to the host.  result() waits for them
    (an event, not the device) and returns (names, numels, TENSOR_ROW_DTYPE rows, watch names, WATCH_ROW_DTYPE rows, the GLOBAL_DTYPE
    words of that step)."""

    def __init__(self, names, numels, watch_names, rows, wrows, glob, done=None):
        self.names, self.numels, self.watch_names = list(names), [int(n) for n in numels], list(watch_names)
        self._rows, self._wrows, self._glob, self._done = rows, wrows, glob, done

    def result(self):
        if self._done is not None:
            self._done.synchronize()
            blob, (a, b, _) = self._rows.numpy(), self._wrows
            self._rows, self._wrows = blob[:a].view(TENSOR_ROW_DTYPE).copy(), blob[a:a + b].view(WATCH_ROW_DTYPE).copy()
            self._glob = blob[a + b:].view(GLOBAL_DTYPE)[0].copy()
            self._done = None
        return self.names, self.numels, self._rows, self.watch_names, self._wrows, self._glob


def make_adam(params, cfg, modules, saved=None):
    """The trainers' optimiser: torch.optim.Adam(params, lr=cfg.lr) as the reference has it, or - cfg.fused_optim, or a cfg.max_grad_norm,
    a cfg.ema_decay or a cfg.tensor_stats, which imply it - FusedAdam over the same parameters and lr, watching the float buffers of the
    trained `modules`.  saved: {stem: module} of the checkpoint files the trainer writes ({stem}_{epoch}.th = module.state_dict()); with
    cfg.tensor_stats every parameter and watched buffer is named "{stem}/{state_dict key}" after the first of them that holds it."""
    params = list(params)
    stats = int(getattr(cfg, "tensor_stats", 0) or 0)
    if not (getattr(cfg, "fused_optim", False) or getattr(cfg, "max_grad_norm", None) or getattr(cfg, "ema_decay", None) or stats):
        return torch.optim.Adam(params, lr=cfg.lr)
    seen, watch = set(), []
    for m in modules:
        for b in m.buffers():
            if b.dtype == torch.float32 and id(b) not in seen:
                seen.add(id(b))
                watch.append(b)
    names = None
    if stats:
        known = {}
        for stem, module in (saved or {}).items():
            for key, t in module.state_dict(keep_vars=True).items():
                known.setdefault(id(t), f"{stem}/{key}")
        names = ([known.get(id(p), f"unsaved/parameter{i}") for i, p in enumerate(params)],
                 [known.get(id(b), f"unsaved/buffer{i}") for i, b in enumerate(watch)])
    return FusedAdam(params, lr=cfg.lr, max_grad_norm=getattr(cfg, "max_grad_norm", None) or None, watch=watch,
                     ema_decay=getattr(cfg, "ema_decay", None) or None, names=names)


def ema_state_dict(module, optimizer):
    """module.state_dict() with every parameter that has a shadow in `optimizer` (FusedAdam(ema_decay=)) replaced by a copy of it.  A
    parameter without one - frozen, or never stepped - stays live, and so does every buffer (BatchNorm's running statistics and
    num_batches_tracked are the live model's: "buffers: live")."""
    sd = module.state_dict()
    for name, p in module.named_parameters(remove_duplicate=False):
        e = optimizer.state.get(p, {}).get("ema")
        if e is not None and name in sd:
            sd[name] = e.detach().clone().view_as(p)
    return sd
