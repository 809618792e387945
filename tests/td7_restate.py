"""The fp64 restatement of a TD7 update and its yardsticks (test infrastructure,
shared by tests/test_td7_full.py, tests/test_td7_restate.py and
tests/test_fused_train_parity_gpu.py).

* TD7Learner on torch-CPU in float64 is the reference of one update;
  _rounded_matmuls routes its GEMMs through _RoundedGemm, which rounds the
  operands to bf16 / fp16 where the HIP kernels do.
* Restatement holds the CPU learners of one case, teacher-forced from another
  learner's state before every phase, and measures per gradient tensor
    noise = rel(fp32 CPU learner, fp64 CPU learner)
    flip  = rel(fp32-accumulating rounded restatement, fp64-accumulating one)
  -- both on the reference alone, never on the kernels.
* unblock_xt decodes a td7f_xt weight-gradient operand (csrc/td7_fused.h
  blk8 / blk4) into a dense matrix.
* td7_batch is helpers.td7_full_batch for any batch size.
"""
import functools

import numpy as np
import torch

from helpers import TD7_FULL_LEARNING_STEPS
from exo_amd import ops
from exo_amd.td7 import Critic, Hyperparameters, TD7Learner

TOL = {"fp32": dict(grad=1e-4, delta=1e-3, prio=1e-5, bound=1e-5, mask=0.02),
       "bf16": dict(grad=1e-2, golden=3e-2, delta=0.15, prio=1e-3, bound=1e-3, mask=0.1),
       "fp16": dict(grad=1e-2, golden=3e-2, delta=0.15, prio=1e-3, bound=1e-3, mask=0.1)}
COND = 4.0  # bounds scale with the reference's own fp32 deviation from fp64 ("noise")
# sqrt(u / eps32) with eps32 = 1e-7 (fp32-level perturbation): bf16 u = 2^-9, fp16 u = 2^-11
AMP = {"fp32": 1.0, "bf16": (2.0 ** -9 / 1e-7) ** 0.5, "fp16": (2.0 ** -11 / 1e-7) ** 0.5}
ROUND = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
NETS = ("actor", "critic", "encoder", "actor_target", "critic_target", "fixed_encoder", "fixed_encoder_target")


def _named(mod, mname, grad=False):
    """Reference-named flat tensors of a module (the critic's stacked heads split)."""
    out = {}
    if isinstance(mod, Critic):
        for k, names in enumerate(Critic.HEADS):
            for what in ("weight", "bias"):
                p = getattr(mod, f"{'w' if what == 'weight' else 'b'}{k}")
                t = p.grad if grad else p
                for h, n in enumerate(names):
                    out[f"{mname}.{n}.{what}"] = None if t is None else t[h]
        return out
    for n, p in mod.named_parameters():
        out[f"{mname}.{n}"] = p.grad if grad else p
    return out


def _rel(x, ref):
    d = np.linalg.norm(ref.astype(np.float64))
    return np.linalg.norm((x - ref).astype(np.float64)) / max(d, 1e-30)


class _RoundedGemm(torch.autograd.Function):
    """y = x @ w^T (+ b) with x, w rounded to `dt` (batched if 3-D); backward
    with dY rounded for both GEMMs (fp16: after scaling by 2^10), the bias
    gradient from the unrounded dY -- the reduced-precision td7_dense kernels'
    arithmetic, in float64."""

    @staticmethod
    def forward(ctx, x, w, b, dt):
        r = lambda t: t.to(dt).to(t.dtype)  # noqa: E731
        ctx.save_for_backward(x, w)
        ctx.dt, ctx.has_b = dt, b is not None
        y = r(x) @ r(w).transpose(-1, -2)
        return y + b.unsqueeze(-2) if b is not None else y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = lambda t: t.to(ctx.dt).to(t.dtype)  # noqa: E731
        gs = 1024.0 if ctx.dt == torch.float16 else 1.0  # fp16: dP scaled by 2^10 before rounding (grad_scale)
        rdy = (dy * gs).to(ctx.dt).to(dy.dtype) / gs
        dx = rdy @ r(w)
        xx = x if x.dim() == dy.dim() else x.unsqueeze(0).expand(dy.shape[0], *x.shape)
        dw = rdy.transpose(-1, -2) @ r(xx)
        if dw.dim() > w.dim():
            dw = dw.sum(0)
        if dx.dim() > x.dim():
            dx = dx.sum(0)
        db = dy.sum(-2) if ctx.has_b else None
        if db is not None and db.dim() > 1 and w.dim() == 2:
            db = db.sum(0)
        return dx, dw, db, None


class _rounded_matmuls:
    """Route the CPU path's F.linear / torch.baddbmm / torch.bmm through _RoundedGemm."""

    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        import torch.nn.functional as F
        self.saved = (F.linear, torch.baddbmm, torch.bmm)
        dt = self.dt
        F.linear = lambda x, w, b=None: _RoundedGemm.apply(x, w, b, dt)
        torch.baddbmm = lambda b, x, wt: _RoundedGemm.apply(x, wt.transpose(1, 2), b.squeeze(1), dt)
        torch.bmm = lambda x, wt: _RoundedGemm.apply(x, wt.transpose(1, 2), None, dt)

    def __exit__(self, *a):
        import torch.nn.functional as F
        F.linear, torch.baddbmm, torch.bmm = self.saved


def _cpu_learner(hp, qbounds=None, seed=0):
    """TD7Learner on torch-CPU in fp32 (torch.optim.Adam), seeded; qbounds:
    the Q-target clamp (min_target, max_target) -- 0 / 0 until the first target
    refresh otherwise, which would hide the clamp."""
    torch.manual_seed(seed)
    L = TD7Learner(80, 7, hp, learning_steps=TD7_FULL_LEARNING_STEPS, device="cpu", fused_adam=False)
    if qbounds is not None:
        L.min_target.fill_(qbounds[0])
        L.max_target.fill_(qbounds[1])
    return L


def _f64_learner(hp, qbounds=(0.0, 0.0), seed=0):
    """A float64 TD7Learner on the CPU (torch.optim.Adam, scalar state in fp64)."""
    L = _cpu_learner(hp, seed=seed)
    for name in NETS:
        getattr(L, name).double()
    L.actor_optimizer = torch.optim.Adam(L.actor.parameters(), lr=L.hp.actor_lr, weight_decay=1e-7)
    L.critic_optimizer = torch.optim.Adam(L.critic.parameters(), lr=L.hp.critic_lr, weight_decay=1e-7)
    L.encoder_optimizer = torch.optim.Adam(L.encoder.parameters(), lr=L.hp.encoder_lr, weight_decay=1e-7)
    f64 = dict(dtype=torch.float64)
    L.max, L.min = torch.tensor(-1e8, **f64), torch.tensor(1e8, **f64)
    L.min_target, L.max_target = torch.tensor(qbounds[0], **f64), torch.tensor(qbounds[1], **f64)
    L.target_policy_noise = L.target_policy_noise.double()
    return L


def _copy_state(dst, src):
    """dst (fp64 CPU learner) <- src's weights and running scalars."""
    with torch.no_grad():
        for name in NETS:
            for p, q in zip(getattr(dst, name).parameters(), getattr(src, name).parameters()):
                p.copy_(q.detach().double().cpu())
        for k in ("max", "min", "min_target", "max_target", "target_policy_noise"):
            getattr(dst, k).copy_(getattr(src, k).detach().double().cpu())
    dst.training_steps = src.training_steps


# ---------------------------------------------------------------------------
# the weight-gradient operands
def xt_index(rows64, ld, precision):
    """[rows64, ld] int64: where element (operand row c, batch row r) of a
    td7f_xt operand lives in its buffer (csrc/td7_fused.h blk8 / blk4), in
    elements of the operand type."""
    c = torch.arange(rows64, dtype=torch.int64)[:, None]
    r = torch.arange(ld, dtype=torch.int64)[None, :]
    if precision == "fp32":  # 1 KiB blocks of 16 operand rows x 16 batch rows, 4 batch rows per lane
        return ((c // 16) * (ld // 16) + r // 16) * 256 + ((c % 16) + 16 * ((r % 16) // 4)) * 4 + r % 4
    return ((c // 16) * (ld // 32) + r // 32) * 512 + ((c % 16) + 16 * ((r % 32) // 8)) * 8 + r % 8


def unblock_xt(buf, rows64, ld, precision):
    """A td7f_xt operand buffer (exo_amd/fused.py XTBuffers.x / .dp: int16 bit
    storage at 16-bit precisions, float32 at fp32) as a dense [rows64, ld]
    float64 tensor on the CPU: operand rows x batch rows."""
    flat = buf.detach().reshape(-1).cpu()
    assert flat.numel() == rows64 * ld, (flat.numel(), rows64, ld)
    if precision != "fp32":
        assert flat.dtype == torch.int16
        flat = flat.view(ROUND[precision])
    else:
        assert flat.dtype == torch.float32
    return flat[xt_index(rows64, ld, precision)].double()


# ---------------------------------------------------------------------------
# batches and learners of the ragged-batch cases
def td7_batch(B, step):
    """helpers.td7_full_batch for any B: (state, action, next_state, reward,
    not_done, noise) from a PCG64 stream keyed by (B, step); rewards in
    [-2, 3], not_done zero on ~10 % of the rows."""
    rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([int(B), int(step)])))
    s = rng.normal(0, 1, (B, 80)).astype(np.float32)
    a = rng.uniform(-1, 1, (B, 7)).astype(np.float32)
    s2 = (s + 0.1 * rng.normal(0, 1, (B, 80))).astype(np.float32)
    r = rng.uniform(-2, 3, (B, 1)).astype(np.float32)
    nd = (rng.uniform(0, 1, (B, 1)) > 0.1).astype(np.float32)
    nz = rng.normal(0, 1, (B, 7)).astype(np.float32)
    return s, a, s2, r, nd, nz


def width_hp(width):
    """Hyperparameters at the default widths (zs / enc 300, critic / actor 320:
    5 tiles per wave) or with every width `width`."""
    if width is None:
        return Hyperparameters()
    return Hyperparameters(zs_dim=width, enc_hdim=width, critic_hdim=width, actor_hdim=width)


def perturbed_cpu_learner(hp, qbounds=None):
    """The cases' initial state: a seeded fp32 CPU learner with the target /
    fixed nets and the actor moved off their copies (as tests/test_fused_gpu.py
    _learner does on the device), so that no two nets share weights."""
    L = _cpu_learner(hp, qbounds, seed=3)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for m in (L.actor_target, L.critic_target, L.fixed_encoder_target, L.fixed_encoder, L.actor):
            for p in m.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.02)
    return L


class _capture:
    """Record what the CPU update's ops.q_target / ops.critic_loss saw: the
    target critic's heads and (Q, Q_target)."""

    def __enter__(self):
        self.saved = (ops.q_target, ops.critic_loss)
        q_target, critic_loss = self.saved

        def qt(heads, *a, **k):
            self.heads = heads.detach().double()
            return q_target(heads, *a, **k)

        def cl(q, q_target_, *a, **k):
            self.td = (q.detach().double() - q_target_.detach().double()).abs()
            return critic_loss(q, q_target_, *a, **k)

        ops.q_target, ops.critic_loss = qt, cl
        return self

    def __exit__(self, *a):
        ops.q_target, ops.critic_loss = self.saved


class Restatement:
    """The CPU learners of one (Hyperparameters, precision) case, reloaded
    from a learner's state before every phase (teacher forcing):
      f32, f64   the plain CPU learner in fp32 and in fp64          -> noise
      r32, r64   the same under _rounded_matmuls(ROUND[precision])  -> flip
                 (16-bit precisions only)
    ref is the fp64 restatement the kernels are compared with (r64, or f64 at
    fp32).  After critic(): td [B, 2] = |Q - Q_target| and heads [B, 2] (the
    target critic's outputs) of ref."""

    def __init__(self, hp, precision):
        self.hp, self.precision = hp, precision
        dt = ROUND[precision]
        self.arms = {"f32": (_cpu_learner(hp), torch.float32, None), "f64": (_f64_learner(hp), torch.float64, None)}
        if dt is not None:
            self.arms["r32"] = (_cpu_learner(hp), torch.float32, dt)
            self.arms["r64"] = (_f64_learner(hp), torch.float64, dt)
        self.ref = self.arms["r64" if dt is not None else "f64"][0]

    def _run(self, state, fn):
        for key, (L, dtype, dt) in self.arms.items():
            _copy_state(L, state)
            rounding = _rounded_matmuls(dt) if dt is not None else None
            if rounding:
                rounding.__enter__()
            try:
                with _capture() as cap:
                    fn(L, dtype)
            finally:
                if rounding:
                    rounding.__exit__()
            if L is self.ref and hasattr(cap, "td"):
                self.td, self.heads = cap.td, cap.heads

    def _yardsticks(self, mnames):
        g = {key: self.grads(L, mnames) for key, (L, _, _) in self.arms.items()}
        if "f32" not in g:  # the restatement alone (case_qbounds)
            return {}, {}
        noise ={k: _rel(g["f32"][k], v) for k, v in g["f64"].items()}
        if "r64" in g:
            flip = {k: _rel(g["r32"][k], v) for k, v in g["r64"].items()}
        else:
            flip = {k: 0.0 for k in noise}
        return noise, flip

    @staticmethod
    def grads(L, mnames):
        """{reference name: whole gradient tensor, flat float64 numpy}"""
        out = {}
        for mname in mnames:
            for name, t in _named(getattr(L, mname), mname, grad=True).items():
                assert t is not None, f"no gradient for {name}"
                out[name] = t.detach().double().cpu().numpy().reshape(-1).copy()
        return out

    def critic(self, state, batch):
        """phase_grads of the step after `state` on every arm -> (noise, flip)
        of the encoder's and the critic's gradients."""
        def fn(L, dtype):
            b = [torch.tensor(x, dtype=dtype) for x in batch]
            L.training_steps += 1
            L.phase_grads(*b[:5], noise=b[5])
        self._run(state, fn)
        return self._yardsticks(("encoder", "critic"))

    def actor(self, state, batch):
        """phase_actor_grads from `state` (the critic just updated) on every
        arm, fixed_zs recomputed -> (noise, flip) of the actor's gradients."""
        def fn(L, dtype):
            s, a = (torch.tensor(x, dtype=dtype) for x in batch[:2])
            L._fixed_zs = L.fixed_encoder.zs(s).detach()
            L.phase_actor_grads(s, a)
        self._run(state, fn)
        return self._yardsticks(("actor",))


def noise_and_flip(hp, batch, state, precision, phase="critic"):
    """(noise, flip) per gradient tensor of one phase of the step after
    `state` (a learner: weights, running bounds, clamp), on the CPU alone.
    phase "critic": phase_grads (encoder and critic tensors); "actor":
    phase_actor_grads (`state` then holds the updated critic).  flip is zero
    at fp32."""
    R = Restatement(hp, precision)
    return R.critic(state, batch) if phase == "critic" else R.actor(state, batch)


# ---------------------------------------------------------------------------
# the ragged-batch cases of tests/test_fused_train_parity_gpu.py; each B is the
# smallest that reaches its edge: 1 one row; 17 a full 16-row tile plus one row;
# 40 tests/test_wgrad_layout_gpu.py's shape; 250 ld = 256 (exactly 8 k-steps at
# 16 bits), a last tile of 10 rows; 264 ld = 512, a last tile of 8 rows
CASES = [("fp32", None, 17), ("fp32", None, 264), ("fp32", 256, 1), ("fp32", 256, 250),
         ("bf16", None, 1), ("bf16", None, 250), ("bf16", 256, 17), ("bf16", 256, 264),
         ("fp16", None, 17), ("fp16", None, 264), ("fp16", 256, 40), ("fp16", 256, 250)]
STEPS = 2  # the second one updates the actor (policy_freq)
FLIP_CAP = 3e-2  # the 16-bit "golden" tolerance: how far 2 * flip may lift a bound


@functools.lru_cache(maxsize=None)
def case_qbounds(precision, width, B):
    """(min_target, max_target) of a case: the 25 % / 75 % quantiles of the
    min-head target values of its first batch under the restatement from the
    initial state, so that the Q-target clamp binds on about half of the rows
    (the learner's own bounds are 0 / 0 until the first target refresh)."""
    hp = width_hp(width)
    R = Restatement(hp, precision)
    arm = R.arms["r64" if "r64" in R.arms else "f64"]
    R.arms = {"ref": arm}  # the yardstick arms are not needed here
    R.critic(perturbed_cpu_learner(hp), td7_batch(B, 0))
    q = R.heads.min(1)[0]
    return float(torch.quantile(q, 0.25)), float(torch.quantile(q, 0.75))


def clamp_fraction(heads, not_done, qbounds):
    """Fraction of the rows whose target the clamp changes: the min head
    outside [min_target, max_target] on a row that is not terminal."""
    q = heads.min(1)[0]
    hit = ((q < qbounds[0]) | (q > qbounds[1])) & (torch.as_tensor(not_done).reshape(-1) != 0)
    return float(hit.double().mean())
