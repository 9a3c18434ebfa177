"""The per-tensor view and the blame ring (csrc/optim.hip: lav_optim_tensor_stats, lav_optim_blame) against their specifications
lav_amd.train.optim.tensor_stats_numpy and blame_numpy on an MI355X: every integer, every histogram bin and the bit pattern of every
maximum equal, each sum of squares within numel * 2^-53 relative; both entries store into nothing they read; --tensor-stats in a trainer."""
import json

import numpy as np
import pytest
import torch

from lav_amd.train import optim as O
from lav_amd.train import tensor_stats as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64
FLT_MAX = np.float32(3.4028235e38)
# element offsets behind a 16-byte boundary of (g, p, m, v): every byte misalignment {0, 4, 8, 12} of g against every one of the p, m, v
# triple (16-byte accesses behind a head of 0 .. 3 elements, g beside them on 16- or 4-byte loads), then four rows whose p, m, v differ
# (4-byte accesses throughout)
MISALIGN = [(a, b, b, b) for b in range(4) for a in range(4)] + [(0, 1, 2, 3), (1, 2, 3, 0), (2, 3, 0, 1), (3, 0, 1, 2)]


class World:
    """Flat float32 buffers g, p, m, v, e (the EMA shadow) holding every tensor of the table at its misalignment, with slack between
    the tensors and GUARD elements behind the last: the specification's copy, and the same layout in HBM."""

    def __init__(self, chunk, seed=0):
        self.chunk = chunk
        big = [1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 3 * chunk]
        # the nine sizes twice, so that the chunk-sized ones meet 16- and 4-byte paths; then 300 tensors of 1 .. 7 elements: more rows
        # than a workgroup has threads, many of them inside one chunk's neighbourhood of the table
        self.sizes = big + big + [i % 7 + 1 for i in range(300)]
        self.patterns = [MISALIGN[(i + (7 if 9 <= i < 18 else 0)) % len(MISALIGN)] for i in range(len(self.sizes))]
        self.patterns[9 + 6], self.patterns[9 + 7] = MISALIGN[17], MISALIGN[19]       # chunk + 1 and 2 chunk + 5 on 4-byte accesses
        assert sum(self.sizes) < 10 ** 5
        rng = self.rng = np.random.default_rng(seed)
        cur = dict.fromkeys("gpmve", 0)
        self.offsets = []
        for n, (og, op, om, ov) in zip(self.sizes, self.patterns):
            offs = {}
            for k, o in zip("gpmve", (og, op, om, ov, op)):
                offs[k] = (cur[k] + 3) // 4 * 4 + 4 + o        # (a gap of slack in front of every tensor)
                cur[k] = offs[k] + n
            self.offsets.append(offs)
        self.length = max(cur.values()) + GUARD
        sign = lambda n: rng.choice([-1.0, 1.0], n)
        self.flat = {k: np.zeros(self.length, np.float32) for k in "gpmve"}
        self.flat["p"][:] = (np.exp(rng.uniform(np.log(1e-4), np.log(10.0), self.length)) * sign(self.length)).astype(np.float32)
        self.flat["m"][:] = (rng.standard_normal(self.length) * 0.1).astype(np.float32)
        self.flat["v"][:] = np.exp(rng.uniform(np.log(1e-8), np.log(1e-1), self.length)).astype(np.float32)
        self.flat["e"][:] = self.flat["p"]
        self.state = O.new_state(len(self.sizes))
        self.glob = np.zeros(1, O.GLOBAL_DTYPE)
        self.rows = []
        for i, (n, offs) in enumerate(zip(self.sizes, self.offsets)):
            row = {k: self.flat[k][offs[k]:offs[k] + n] for k in "gpmve"}
            row.update(lr=1e-2 * (1 + i % 3), beta1=0.9, beta2=0.999, eps=1e-8, state=i)
            self.rows.append(row)
        # a parameter that is not finite is counted, not hidden; v = 0 under a moment that is not: the largest update there is
        self.rows[5]["p"][[0, chunk - 1]] = [np.nan, -np.inf]
        self.rows[7]["v"][[0, chunk, 2 * chunk + 4]] = 0.0
        self.watch = [np.ones(chunk + 5, np.float32), np.full(3, -7.5, np.float32), np.zeros(5, np.float32)]
        self.watch[0][[0, chunk + 1]] = [np.nan, 1e30]
        self.watch[2][4] = np.inf

    def spots(self, n):
        """The first and the last element of every chunk of a tensor, and the lanes of the 4-byte heads and tails."""
        s = {0, 1, 2, n - 1, n - 2, n - 3}
        for c in range(0, n, self.chunk):
            s |= {c, c + 1, min(c + self.chunk, n) - 1}
        return sorted(i for i in s if 0 <= i < n)

    def draw_gradients(self, bad):
        """Magnitudes 2^-45 .. 2^25, either sign: both end bins fill.  At the spots -0.0, a denormal, +0.0 and - bad: a step that will
        not be applied - NaN, +-Inf and FLT_MAX."""
        n = self.length
        self.flat["g"][:] = (np.exp2(self.rng.uniform(-45.0, 25.0, n)) * self.rng.choice([-1.0, 1.0], n)).astype(np.float32)
        values = [-0.0, 1e-40, 0.0] + ([np.nan, np.inf, -np.inf, FLT_MAX, -FLT_MAX] if bad else [])
        k = 0
        for i, row in enumerate(self.rows):
            if self.sizes[i] > 7 or i % 5 == 0:
                for s in self.spots(self.sizes[i]):
                    row["g"][s] = values[k % len(values)]
                    k += 1
        self.rows[20]["g"][:] = 0.0         # a gradient that is all zero

    def table(self, bases):
        t = np.zeros(len(self.rows), O.TENSOR_DTYPE)
        for i, (row, offs) in enumerate(zip(self.rows, self.offsets)):
            t[i] = tuple(bases[k] + 4 * offs[k] for k in "pgmv") + (self.sizes[i], row["lr"], row["beta1"], row["beta2"], row["eps"], i, 0)
        return t, O.fill_chunks(t, self.chunk)


def _dev(array):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).to(DEV)


class DeviceWorld:
    def __init__(self, seed=0):
        from lav_amd import ops
        self.ops = ops
        self.w = w = World(O.chunk_length(), seed)
        self.flat = {k: torch.from_numpy(w.flat[k].copy()).to(DEV) for k in "gpmve"}
        assert all(t.data_ptr() % 16 == 0 for t in self.flat.values())
        bases = {k: t.data_ptr() for k, t in self.flat.items()}
        table, self.chunks = w.table(bases)
        self.n = len(table)
        self.table = _dev(table)
        self.shadow = _dev(np.asarray([bases["e"] + 4 * offs["e"] for offs in w.offsets], "<u8"))
        # the watched buffers at byte offsets 0, 4 and 12 behind a 16-byte boundary
        self.wflat = torch.zeros(sum(b.size + 8 for b in w.watch), device=DEV)
        wt, at = np.zeros(len(w.watch), O.WATCH_DTYPE), 0
        for r, (b, o) in enumerate(zip(w.watch, (0, 1, 3))):
            at = (at + 3) // 4 * 4 + o
            self.wflat[at:at + b.size] = torch.from_numpy(b)
            wt[r] = (self.wflat.data_ptr() + 4 * at, b.size, 0, 0)
            at += b.size
        self.wchunks = O.fill_chunks(wt, w.chunk)
        self.nw = len(wt)
        self.wtable = _dev(wt)
        self.state, self.glob = _dev(w.state), _dev(w.glob)
        self.rows_out = torch.zeros(self.n * O.TENSOR_ROW_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        self.watch_out = torch.zeros(self.nw * O.WATCH_ROW_DTYPE.itemsize, dtype=torch.uint8, device=DEV)
        self.blame = torch.zeros(O.BLAME_DTYPE.itemsize, dtype=torch.uint8, device=DEV)

    def new_gradients(self, bad):
        self.w.draw_gradients(bad)
        self.flat["g"].copy_(torch.from_numpy(self.w.flat["g"]))

    def step(self):
        """One guarded step with the moving average, here and in the specification; p, m, v, e and the words stay equal in every bit."""
        w = self.w
        self.ops.optim_adam_ema_step(self.table, self.n, self.chunks, self.wtable, self.nw, self.wchunks, self.state, self.glob, self.shadow, 0.99)
        O.fused_adam_numpy(w.rows, w.state, w.glob, watch=w.watch, ema_decay=0.99)
        for k in "pmve":
            assert np.array_equal(self.flat[k].cpu().numpy(), w.flat[k], equal_nan=True), k      # (a NaN's payload is nobody's promise)
        assert np.array_equal(self.state.cpu().numpy(), np.ascontiguousarray(w.state).view(np.uint8))

    def stats(self):
        self.ops.optim_tensor_stats(self.table, self.n, self.chunks, self.wtable, self.nw, self.wchunks, self.state, self.rows_out, self.watch_out)
        return self.rows_out.cpu().numpy().view(O.TENSOR_ROW_DTYPE), self.watch_out.cpu().numpy().view(O.WATCH_ROW_DTYPE)

    def snapshot(self):
        return [t.clone() for t in (*self.flat.values(), self.wflat, self.state, self.glob, self.table, self.wtable)]


def _compare(d, what):
    w = d.w
    got, wgot = d.stats()
    want, wwant = O.tensor_stats_numpy(w.rows, w.state, w.watch)
    for k in ("g_nonfinite", "g_zeros", "p_nonfinite", "hist", "reserved"):
        bad = np.flatnonzero(np.any((got[k] != want[k]).reshape(len(got), -1), axis=1))
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} tensors, first {bad[:3]} (sizes {[w.sizes[i] for i in bad[:3]]}): {got[k][bad[:3]]} != {want[k][bad[:3]]}"
    for k in ("g_maxabs", "p_maxabs", "u_maxabs"):
        bad = np.flatnonzero(got[k].view(np.uint32) != want[k].view(np.uint32))
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} tensors, first {bad[:3]}: {got[k][bad[:3]]!r} != {want[k][bad[:3]]!r}"
    worst = 0.0
    for k in ("g_sumsq", "p_sumsq", "u_sumsq"):
        for i, n in enumerate(w.sizes):
            a, b = float(got[k][i]), float(want[k][i])
            if b == 0.0:
                assert a == 0.0, f"{what}: {k}[{i}] is {a!r}, the specification's is 0"
            else:
                worst = max(worst, abs(a - b) / b / (n * 2.0 ** -53))
                assert abs(a - b) <= n * 2.0 ** -53 * b, f"{what}: {k}[{i}] {a!r} != {b!r} ({n} elements)"
    assert wgot.tobytes() == wwant.tobytes(), f"{what}: buffers {wgot} != {wwant}"
    print(f"{what}: equal; worst sumsq distance {worst:.3f} of its bound; bins 0 / 63 hold {int(want['hist'][:, 0].sum())} / {int(want['hist'][:, 63].sum())}; "
          f"g_nonfinite {int(want['g_nonfinite'].sum())}, u_maxabs up to {float(want['u_maxabs'].max()):.3e}")
    return want


def test_kernel_equals_the_specification_and_stores_nothing():
    """The table of the module's World (two times 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 5, 3 chunk, then 300 tensors of 1 .. 7
    elements; g against the p, m, v triple at all 16 pairs of byte misalignments, and p, m, v apart) and three watched buffers, compared
    before any step on gradients holding NaN, +-Inf, +-FLT_MAX, -0.0 and a denormal at the first and last element of every chunk and in
    the head and tail lanes; after 1 and after 3 applied steps (a tensor at step 0 gives u = 0, then u is the step's own term); after one
    skipped step on such gradients again.  Around the last comparison's launches and a blame launch the whole backing buffers of g, p,
    m, v and the EMA shadow (slack and guard included), the watched buffers, the words and the tables keep every byte."""
    d = DeviceWorld()
    d.new_gradients(bad=True)
    want = _compare(d, "before any step")
    assert want["hist"][:, 0].sum() > 0 and want["hist"][:, 63].sum() > 0 and want["g_nonfinite"].sum() > 0 and want["u_maxabs"].max() == 0
    assert want["p_nonfinite"][5] == 2 and want["g_zeros"][20] == d.w.sizes[20]
    for steps in (1, 3):
        while int(d.w.glob[0]["applied"]) < steps:
            d.new_gradients(bad=False)
            d.step()
        want = _compare(d, f"after {steps} applied steps")
        assert int(d.w.state["step"].min()) == steps and want["u_maxabs"].min() >= 0 and want["u_sumsq"][7] > 0 and want["g_nonfinite"].sum() == 0
    d.new_gradients(bad=True)
    u_before = (want["u_sumsq"].copy(), want["u_maxabs"].copy())
    d.step()
    assert int(d.w.glob[0]["skipped"]) == 1 and int(d.w.glob[0]["applied"]) == 3
    before = d.snapshot()
    want = _compare(d, "after a skipped step")
    assert np.array_equal(want["u_sumsq"], u_before[0]) and np.array_equal(want["u_maxabs"], u_before[1])       # the previous applied update
    d.ops.optim_blame(d.table, d.n, d.chunks, d.wtable, d.nw, d.wchunks, d.glob, d.blame)
    torch.cuda.synchronize()
    for a, b in zip(before, d.snapshot()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    host = np.zeros(1, O.BLAME_DTYPE)
    O.blame_numpy(d.w.rows, d.w.glob, host, d.w.watch)
    assert d.blame.cpu().numpy().tobytes() == host.tobytes() and host["written"][0].tolist() == [4, 2]


def _blame_sequence(make, poison, step):
    """The sequence of tests/test_tensor_stats_host.py: an applied step, then five skipped ones (bad gradients in tensors 2, 5, 6, 7, 9 -
    three elements in tensor 6), the last three with a watched buffer that is not finite."""
    params, watched, opt = make()
    for s in range(6):
        for i, p in enumerate(params):
            p.grad = torch.full_like(p, 0.25 * (i + 1))
        if s >= 1:
            for i in (2, 5, 6, 7, 9):
                params[i].grad.view(-1)[-1] = float("nan")
            params[6].grad.view(-1)[:2] = float("inf")
        if s >= 3:
            poison(watched)
        step(opt)
    return opt


def test_blame_on_the_device_equals_the_specification():
    """FusedAdam(names=) on cuda parameters against the same sequence through blame_numpy: the block equal in every byte, the ring
    wrapped by the fifth skipped step, the applied step recorded nowhere, the watched buffer named."""
    sizes = [3, 5000, 1, 7, 4096, 2, 9000, 4, 6, 8, 5]

    def make(device):
        params = [torch.nn.Parameter(torch.zeros(n, device=device)) for n in sizes]
        watched = [torch.ones(4, device=device), torch.ones(4100, device=device)]
        return params, watched, O.FusedAdam(params, lr=1e-3, watch=watched, names=([f"t{i}" for i in range(len(sizes))], ["b0", "b1"]))

    def poison(watched):
        watched[1][4099] = float("nan")

    dev = _blame_sequence(lambda: make(DEV), poison, lambda opt: opt.step())
    cpu = _blame_sequence(lambda: make("cpu"), poison, lambda opt: opt.step())
    got, want = dev._blame.cpu().numpy().view(O.BLAME_DTYPE), cpu._blame.numpy().view(O.BLAME_DTYPE)
    assert got.tobytes() == want.tobytes(), (got, want)
    assert got[0]["written"].tolist() == [20, 3] and dev.health()["skipped"] == 5 and dev.health()["applied"] == 1
    tensors, buffers = dev.blame()
    assert [r["ordinal"] for r in tensors] == list(range(4, 20)) and [r["name"] for r in tensors[-4:]] == ["t2", "t5", "t6", "t7"]
    assert [r["nonfinite"] for r in tensors[-4:]] == [1, 1, 3, 1] and [r["step"] for r in tensors[-4:]] == [6] * 4 and tensors[0]["step"] == 3
    assert [(r["name"], r["nonfinite"], r["step"]) for r in buffers] == [("b1", 1, 4), ("b1", 1, 5), ("b1", 1, 6)]


def test_trainer_with_tensor_stats(tmp_path, monkeypatch):
    """The trainer and size of tests/test_gpu_optim.py's test_trainer_with_the_fused_step, three deterministic steps, with
    --tensor-stats 1 as the trainers' main drives it (TensorStatsLog) and without: parameters, moments and the optimiser's words equal
    in every bit; three lines, whose names are keys of the checkpoints the trainer saves; without the flag neither new ops function
    is called."""
    from lav_amd import ops
    from lav_amd.train import LAV, TrainConfig, synthetic_lidar_batch
    from lav_amd.train.run import set_deterministic
    calls = dict(optim_tensor_stats=0, optim_blame=0)
    for name in calls:
        def counted(*a, _f=getattr(ops, name), _n=name, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, counted)
    batches = [synthetic_lidar_batch(2, seed=40 + i, max_points=20000, num_objs=3) for i in range(2)]
    set_deterministic(True)
    try:
        out = []
        for every in (0, 1):
            torch.manual_seed(0)
            lav = LAV(TrainConfig(log_inference=False, fused_optim=True, tensor_stats=every), DEV, what="lidar")
            opt = lav.lidar_optim
            log = T.TensorStatsLog(str(tmp_path), every) if every else None
            for s in range(3):
                torch.manual_seed(1000 + s)
                lav.train_lidar(*batches[s % 2])
                if log is not None:
                    log.after_step(opt, s)
            if log is None:
                assert calls == dict(optim_tensor_stats=0, optim_blame=0) and opt.names is None
            else:
                assert log.digest().startswith("tensor stats it 2: update_ratio max ")
                log.blamed(opt.blame())
                log.close()
            params = [p for g in opt.param_groups for p in g["params"]]
            out.append(([p.detach().clone() for p in params], [opt.state[p][k].clone() for p in params if p in opt.state for k in ("exp_avg", "exp_avg_sq")],
                        opt._rows_host().copy(), opt.health(), {k: lav.state_dict(k) for k in ("lidar", "uniplanner")}))
    finally:
        set_deterministic(False)
    (p0, m0, w0, h0, _), (p1, m1, w1, h1, saved) = out
    assert calls == dict(optim_tensor_stats=3, optim_blame=3)
    assert len(p0) == len(p1) and all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert len(m0) == len(m1) > 100 and all(torch.equal(a, b) for a, b in zip(m0, m1))
    assert w0.tobytes() == w1.tobytes() and h0 == h1 and h1["applied"] == 3 and h1["skipped"] == 0
    lines = [json.loads(x) for x in open(tmp_path / T.FILE)]
    assert [ln["global_it"] for ln in lines] == [0, 1, 2] and all(ln["applied"] for ln in lines)
    for ln in lines:
        assert len(ln["tensors"]) > 100 and len(ln["buffers"]) > 10
        for name in list(ln["tensors"]) + list(ln["buffers"]):
            stem, key = name.split("/", 1)
            assert key in saved[stem], name
        assert abs(sum(t["grad_norm"] ** 2 for t in ln["tensors"].values()) - ln["grad_norm"] ** 2) <= 1e-9 * ln["grad_norm"] ** 2
        assert all(t["grad_nonfinite"] == 0 and sum(t["grad_hist"]["bins"]) == t["numel"] for t in ln["tensors"].values())
