"""Row-tile-fused TD7 networks on the GPU (csrc/td7_fused.hip): the host side.

With bf16 / fp16 MFMA operands -- and exact fp32 ones (v_mfma_f32_16x16x4_f32,
the reference's precision; EXO_FUSED_F32=0 keeps fp32 per layer) -- the TD7 nets of
Agent/TD7_multi_agent.py:61-140 run as whole-network launches (one workgroup
per 16 rows, activations in LDS) instead of one launch per Linear.  Their
weights are read from packed copies in MFMA-fragment order (PackedLinear),
refreshed by td7f_pack after every change of the fp32 master weights
(optimiser steps, target refreshes, loads).

FusedNets owns the packed copies of every net the update reads and the
launch wrappers; TD7Learner routes its passes here when `fused` is on.
"""
import ctypes
import os

import numpy as np
import torch

from . import _native as nat
from . import ops

PD = 5  # include/exo_amd.h TD7F_PD
NW = 4  # waves per fused workgroup (csrc/td7_fused.h)
MAX_PACK = 32
MAX_ADAM_PACK = 16  # include/exo_amd.h TD7F_MAX_ADAM_PACK
PREC = {"bf16": 1, "fp16": 2, "fp32": 3}
# inputs per k-step (64 bytes of a row): 32 16-bit or 16 fp32 operands
KD = {1: 32, 2: 32, 3: 16}
# the fp32 fused path (csrc/td7_fused.h Ty<PREC_F32>): 0.50 vs 0.79 ms per
# configs[1] iteration per layer, parity-tested against the reference golden at
# the fp32 bounds (tests/test_td7_full.py); EXO_FUSED_F32=0 runs fp32 per layer
FUSED_F32 = os.environ.get("EXO_FUSED_F32", "1") == "1"


TD7FLin, TD7FPackJob, TD7FNoise = nat.TD7FLin, nat.TD7FPackJob, nat.TD7FNoise


def _ks(k, kd=32):
    """k-steps of a packed operand: ceil(k / kd) rounded up to TD7F_PD."""
    return -(-(-(-k // kd)) // PD) * PD


def _etype(prec):
    """torch dtype of an operand-type buffer (bit storage)."""
    return torch.float32 if prec == 3 else torch.int16


def _tiles(n):
    """16-wide tiles of a packed operand: exact up to NW, else a multiple of NW."""
    t = -(-n // 16)
    return t if t <= NW else -(-t // NW) * NW


class PackedLinear:
    """The packed operands of one Linear W [N, K] (a view of the fp32 master
    weight; one head of a stacked critic layer is a slice) in the operand type
    of prec: the forward operand and, with bwd=True, the dX operand (16 bytes
    per lane per 64-lane block either way)."""

    def __init__(self, weight, bias, bwd, prec=1):
        N, K = weight.shape
        dev = weight.device
        kd = KD[prec]
        self.weight, self.bias = weight, bias
        self.N, self.K = N, K
        self.ksf, self.ntf = _ks(K, kd), _tiles(N)
        self.wf = torch.zeros(self.ntf * self.ksf * 64 * 8, dtype=torch.int16, device=dev)
        self.ksb = _ks(N, kd) if bwd else 0
        self.ntb = -(-(-(-K // 16)) // NW) * NW if bwd else 0
        self.wb = torch.zeros(self.ntb * self.ksb * 64 * 8, dtype=torch.int16, device=dev) if bwd else None
        assert weight.stride(1) == 1
        self.lin = TD7FLin(self.wf.data_ptr(), self.wb.data_ptr() if bwd else None, bias.data_ptr(), N, K, self.ksf,
                           self.ksb, weight.data_ptr(), weight.stride(0))

    def job(self):
        w = self.weight
        assert w.stride(1) == 1
        return TD7FPackJob(w.data_ptr(), w.stride(0), self.N, self.K, self.wf.data_ptr(),
                           self.wb.data_ptr() if self.wb is not None else None, self.ksf, self.ntf, self.ksb, self.ntb)


def _lin_array(lins):
    return (TD7FLin * len(lins))(*[pl.lin for pl in lins])


class PackedNet:
    """Packed copies of a set of Linears, refreshed together by one td7f_pack launch."""

    def __init__(self, layers, prec, bwd=False):
        self.layers = [PackedLinear(w, b, bwd, prec) for w, b in layers]
        self.prec = prec
        self.array = _lin_array(self.layers)

    def pack(self, stream=None):
        jobs = [pl.job() for pl in self.layers]
        dev = self.layers[0].wf.device
        st = stream if stream is not None else nat.stream_ptr(dev)
        for i in range(0, len(jobs), MAX_PACK):
            part = jobs[i:i + MAX_PACK]
            nat.check(nat.lib().td7f_pack(self.prec, len(part), (TD7FPackJob * len(part))(*part), st), "td7f_pack")
        self._ver = self._versions()

    def _versions(self):
        return tuple(t._version for pl in self.layers for t in (pl.weight, pl.bias))

    def refresh(self):
        """Repack when a master weight changed through torch since the last
        pack (load_state_dict, copy_: their version counters moved); the HIP
        optimiser steps write the masters in place, and their callers repack
        explicitly (TD7Learner.phase_actor_step, maybe_update_targets)."""
        if self._versions() != self._ver:
            self.pack()


def encoder_layers(enc):
    return [(getattr(enc, n).weight, getattr(enc, n).bias) for n in ("zs1", "zs2", "zs3", "zsa1", "zsa2", "zsa3")]


def actor_layers(actor):
    return [(getattr(actor, n).weight, getattr(actor, n).bias) for n in ("l0", "l1", "l2", "l3")]


def critic_layers(critic):
    """[layer][head] order: w_k[h] of the stacked critic (the reference's q01/q02, q1/q4, q2/q5, q3/q6)."""
    out = []
    for k in range(4):
        w, b = getattr(critic, f"w{k}"), getattr(critic, f"b{k}")
        for h in range(2):
            out.append((w[h], b[h]))
    return out


def supported(learner):
    """The fused path applies: GPU, bf16/fp16/fp32 operands (fp32 unless
    EXO_FUSED_F32=0), the reference's activations, and every hidden width
    (zs_dim, enc_hdim, critic_hdim, actor_hdim) a multiple of 4 in 241..320 --
    16-wide tiles per wave of 4 or 5 (NW = 4 waves), all widths in the same
    tile class.  Anything else (the wide configuration, widths below 241)
    runs the per-layer kernels."""
    hp = learner.hp
    if learner.device.type != "cuda" or learner.precision not in PREC:
        return False
    if learner.precision == "fp32" and not FUSED_F32:
        return False
    acts = [ops.act_code(f) for f in (hp.enc_activ, hp.actor_activ, hp.critic_activ)]
    if any(a is None or a == ops.ACT_CODES["tanh"] for a in acts):
        return False
    widths = (hp.zs_dim, hp.enc_hdim, hp.critic_hdim, hp.actor_hdim)
    th = {_tiles(w) // NW for w in widths}
    return all(49 <= w <= 320 and w % 4 == 0 for w in widths) and len(th) == 1 and th <= {4, 5}


class PlanError(RuntimeError):
    """A network shape the fused passes' shared-memory plan cannot hold."""


class FusedNets:
    """Packed copies of every TD7 net plus the fused launches of one learner."""

    def __init__(self, learner):
        L = learner
        self.L = L
        self.prec = PREC[L.precision]
        self.dev = L.device
        hp = L.hp
        self.act = (ctypes.c_int32 * 3)(ops.act_code(hp.enc_activ), ops.act_code(hp.actor_activ),
                                        ops.act_code(hp.critic_activ))
        self._build()
        self.probe()

    @torch.no_grad()
    def probe(self):
        """Every fused pass once in plan-only mode (td7f_probe: arguments and
        the LDS plan checked, nothing launched) at the row counts whose plans
        differ (select's 16- and 32-row tiles), when the learner builds its
        passes instead of at the first call of a pass that cannot run (ADVICE
        r4: fp32 with zs_dim well above actor_hdim).  An inference pass
        (select_action, the target heads, the fixed embeddings) that does not
        fit raises PlanError: the learner keeps the per-layer kernels.  A
        gradient pass that does not (the actor passes need hidden widths in
        multiples of 16: the Pink agent's 300-wide actor) leaves train_ok
        False: fused inference, per-layer update (TD7Learner.fused_train)."""
        L, dev = self.L, self.dev
        S, A = L.actor.l0.in_features, L.actor.l3.out_features
        B = 16
        # FusedTrain points the parameters' .grad at its own buffers: restored after
        params = [p for m in (L.encoder, L.critic, L.actor) for p in m.parameters()]
        grads = [p.grad for p in params]
        f32 = dict(dtype=torch.float32, device=dev)
        lib = nat.lib()
        lib.td7f_probe(1)
        self.train_ok = False
        try:
            s, a = torch.zeros((B, S), **f32), torch.zeros((B, A), **f32)
            try:
                for n in (B, 8200):
                    self.select(torch.zeros((n, S), **f32))
                self.target_heads(s, noise=torch.zeros((B, A), **f32))
                zs, zsa = self.fixed(s, a)
            except RuntimeError as e:
                raise PlanError(f"fused TD7 passes: {e}") from e
            try:
                t = FusedTrain(self, B)
                one = torch.zeros((B, 1), **f32)
                t.encoder(s, a, s)
                for ph in (0, 1, 2):
                    t.critic(s, a, zs, zsa, torch.zeros((B, 2), **f32), one, one, phase=ph)
                for ph in (0, 1, 2):
                    t.actor(ph, s, zs)
                for ph in (1, 2):  # the offline (TD3+BC) variants
                    t.actor(ph, s, zs, action=a, lmbda=0.1)
                self.train_ok = True
            except RuntimeError as e:  # inference fused, the update per layer
                self.train_error = str(e)
        finally:
            lib.td7f_probe(0)
            for p, g in zip(params, grads):
                p.grad = g

    def _build(self):
        L, p = self.L, self.prec
        self.nets = {
            "fixed_encoder": PackedNet(encoder_layers(L.fixed_encoder), p, bwd=True),
            "fixed_encoder_target": PackedNet(encoder_layers(L.fixed_encoder_target), p),
            "actor": PackedNet(actor_layers(L.actor), p, bwd=True),
            "actor_target": PackedNet(actor_layers(L.actor_target), p),
            "critic_target": PackedNet(critic_layers(L.critic_target), p),
            "encoder": PackedNet(encoder_layers(L.encoder), p, bwd=True),
            "critic": PackedNet(critic_layers(L.critic), p, bwd=True),
        }
        self.pack_all()
        self._train = {}

    def train(self, B):
        """The gradient passes for batches of B rows (buffers made on first use)."""
        t = self._train.get(B)
        if t is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedNets.train: run once eagerly before graph capture")
            t = self._train[B] = FusedTrain(self, B)
        return t

    def rebuild(self):
        """After the learner re-created nets (Agent.load): new views, repacked."""
        self._build()

    def pack(self, *names):
        """Repack the named nets in as few td7f_pack launches as their layers fit
        (TD7F_MAX_PACK jobs each)."""
        nets = [self.nets[n] for n in names]
        jobs = [pl.job() for net in nets for pl in net.layers]
        st = nat.stream_ptr(self.dev)
        for i in range(0, len(jobs), MAX_PACK):
            part = jobs[i:i + MAX_PACK]
            nat.check(nat.lib().td7f_pack(self.prec, len(part), (TD7FPackJob * len(part))(*part), st), "td7f_pack")
        for net in nets:
            net._ver = net._versions()

    def pack_all(self):
        self.pack(*self.nets)

    def adam_pack(self, opts, *names):
        """FlatAdam.step_many(opts) followed by pack(*names), as one
        td7f_adam_pack launch: the thread that updates a weight writes its
        packed copies.  Every packed weight must be a parameter (or a head of
        one) of one of the optimisers; one without a gradient is not stepped
        and keeps its packed copy."""
        from .td7 import FlatAdam
        segs = FlatAdam.segments(opts)
        if not segs:
            return
        nets = [self.nets[n] for n in names]
        jobs, jseg = [], []
        for net in nets:
            for pl in net.layers:
                ptr = pl.weight.data_ptr()
                for k, o in enumerate(opts):
                    e = (ptr - o.flat.data_ptr()) // 4
                    if 0 <= e < o.flat.numel():
                        break
                else:
                    raise ValueError("adam_pack: a packed weight outside the optimisers' parameters")
                hit = [i for i, sg in enumerate(segs) if sg[3] == k and sg[1] <= e < sg[1] + sg[2]]
                if hit:
                    jobs.append(pl.job())
                    jseg.append(hit[0])
        if (len(opts) > FlatAdam.MAX_OPT or len(segs) > FlatAdam.MAX_SEG or len(jobs) > MAX_ADAM_PACK
                or not all(pl.weight.is_contiguous() for net in nets for pl in net.layers)):
            FlatAdam.step_many(opts)
            self.pack(*names)
            return
        nj = len(jobs)
        extra = (nj, (TD7FPackJob * nj)(*jobs), (ctypes.c_int32 * nj)(*jseg))
        nat.check(nat.lib().td7f_adam_pack(self.prec, *FlatAdam.multi_args(opts, segs, extra)), "td7f_adam_pack")
        for net in nets:
            net._ver = net._versions()

    def refresh(self, *names):
        for n in names:
            self.nets[n].refresh()

    # ------------------------------------------------------------- noise
    def _noise(self, rng, sigma, dec, clip, scale, z=None, dec_count=None):
        return TD7FNoise(rng.seed, rng.tag, 0, rng.counter_ptr, rng.ticket_ptr, sigma.data_ptr(), float(dec),
                         float(clip), float(scale), 0, z.data_ptr() if z is not None else None,
                         dec_count.data_ptr() if dec_count is not None else None)

    # ------------------------------------------------------------- passes
    def zs_image(self, n):
        """the [n][zs_dim] operand-type buffer select_zs fills (allocated on the
        first call, which must come before any graph capture that uses it)"""
        Z = self.L.hp.zs_dim
        buf = getattr(self, "_zs_img", None)
        if buf is None or buf.shape[0] < n:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedNets.zs_image: allocate it eagerly before graph capture")
            buf = self._zs_img = torch.empty((n, Z), dtype=_etype(self.prec), device=self.dev)
        return buf[:n]

    @torch.no_grad()
    def select_zs(self, obs, wg_cap=None, rt=None):
        """The fixed encoder's half of select (td7f_select_part mode 1):
        fixed_encoder.zs(obs) (TD7_multi_agent.py:93-97), normalised, into
        zs_image(n) -- no actor, no noise, no exploration-state change.  The
        fixed encoder changes only at target refreshes, so a training loop can
        run this as soon as the observations exist and the actor half, select
        (..., zs_img=), after the actor step: the pair is select bit for bit
        (same rt)."""
        self.refresh("fixed_encoder")
        obs = obs.contiguous()
        n = obs.shape[0]
        img = self.zs_image(n)
        fe = self.nets["fixed_encoder"].layers
        nat.check(nat.lib().td7f_select_part(self.prec, self.act, _lin_array(fe[:3]), self.nets["actor"].array,
                                             nat.ptr(obs), n, None, None, int(wg_cap or 0), int(rt or 0),
                                             nat.ptr(img), 1, nat.stream_ptr(obs.device)), "td7f_select_part")
        return img

    @torch.no_grad()
    def select(self, obs, scale=1.0, dec_count=None, world=1, wg_cap=None, rt=None, zs_img=None, pink=None):
        """select_action_batch with Gaussian exploration (one launch): actor(obs,
        fixed_encoder.zs(obs)) + N(0, exploration_noise) per element, clamped,
        times max_action; exploration_noise decreases once per env (dec_count:
        an int32 device scalar -- once per env counted there, the active envs
        of a vectorised step; times `world`, the data-parallel ranks stepping
        as many envs each).  pink (a PinkNoise.for_learner of these n envs):
        instead of the Gaussian draw, row r adds column t[r] of its own
        coloured sequence (td7f_select_seq, still one launch; with zs_img its
        mode 2) and the noise state the PinkNoise is bound to decreases once
        per call (TD7_multi_agent_Pink_noise.py:218-226); dec_count and world
        do not apply."""
        L = self.L
        self.refresh(*(("actor",) if zs_img is not None else ("fixed_encoder", "actor")))
        obs = obs.contiguous()
        n = obs.shape[0]
        out = torch.empty((n, L.actor.l3.out_features), dtype=torch.float32, device=obs.device)
        if pink is not None:
            if pink.K != 1 or pink.n != n or pink.A != out.shape[1] or pink.dev != obs.device:
                raise ValueError(f"FusedNets.select: the PinkNoise holds {pink.K} policies, {pink.n} envs of "
                                 f"{pink.A} actions on {pink.dev}; the call has 1, {n}, {out.shape[1]} on {obs.device}")
            nz = pink.noise(scale)
            fe = self.nets["fixed_encoder"].layers
            nat.check(nat.lib().td7f_select_seq(self.prec, self.act, _lin_array(fe[:3]), self.nets["actor"].array,
                                                nat.ptr(obs), n, ctypes.byref(nz), nat.ptr(pink.seq), nat.ptr(pink.t),
                                                pink.Lmax, nat.ptr(out), int(wg_cap or 0), int(rt or 0),
                                                nat.ptr(zs_img), 2 if zs_img is not None else 0,
                                                nat.stream_ptr(obs.device)), "td7f_select_seq")
            return out
        dec = L.action_noise_decrease * world
        if dec_count is not None:
            nz = self._noise(L._explore_rng, L.exploration_noise_t, dec, 0.0, scale, dec_count=dec_count)
        else:
            nz = self._noise(L._explore_rng, L.exploration_noise_t, dec * n, 0.0, scale)
        fe, ac = self.nets["fixed_encoder"].layers, self.nets["actor"].layers
        # wg_cap: at most this many workgroups per launch (None / 0: one launch);
        # rt: rows per tile / 16 (None / 0: the library's pick)
        if zs_img is not None:  # the actor half after select_zs (td7f_select_part mode 2)
            nat.check(nat.lib().td7f_select_part(self.prec, self.act, _lin_array(fe[:3]), self.nets["actor"].array,
                                                 nat.ptr(obs), n, ctypes.byref(nz), nat.ptr(out), int(wg_cap or 0),
                                                 int(rt or 0), nat.ptr(zs_img), 2, nat.stream_ptr(obs.device)),
                      "td7f_select_part")
            return out
        nat.check(nat.lib().td7f_select(self.prec, self.act, _lin_array(fe[:3]), self.nets["actor"].array,
                                        nat.ptr(obs), n, ctypes.byref(nz), nat.ptr(out), int(wg_cap or 0),
                                        int(rt or 0), nat.stream_ptr(obs.device)), "td7f_select")
        return out

    def _img(self, B):
        Z = self.L.hp.zs_dim
        A = self.L.actor.l3.out_features
        buf = getattr(self, "_tgt_img", None)
        if buf is None or buf.shape[0] < B:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedNets.target: run once eagerly before graph capture")
            buf = self._tgt_img = torch.empty((B, -(-(2 * Z + A) // 8) * 8), dtype=_etype(self.prec), device=self.dev)
        return buf

    @torch.no_grad()
    def target_heads(self, next_state, noise=None, out=None):
        """Both heads of critic_target(s', a'(s'), zsa', zs') [B, 2] with a' the
        noisy target action (:233-241); two launches.  noise: given standard
        normals [B, A] (parity tests) instead of the device stream.  out: a
        [B, 2] fp32 buffer to write (else a new tensor)."""
        L = self.L
        self.refresh("fixed_encoder_target", "actor_target", "critic_target")
        ns = next_state.contiguous()
        B = ns.shape[0]
        qt = out if out is not None else torch.empty((B, 2), dtype=torch.float32, device=ns.device)
        z = noise.to(device=ns.device, dtype=torch.float32).contiguous() if noise is not None else None
        nz = self._noise(L._noise_rng, L.target_policy_noise, L.policy_noise_decrease, L.hp.noise_clip, 1.0, z)
        nat.check(nat.lib().td7f_target(self.prec, self.act, self.nets["fixed_encoder_target"].array,
                                        self.nets["actor_target"].array, self.nets["critic_target"].array,
                                        nat.ptr(ns), B, ctypes.byref(nz), nat.ptr(self._img(B)), nat.ptr(qt),
                                        nat.stream_ptr(ns.device)), "td7f_target")
        return qt

    @torch.no_grad()
    def fixed(self, state, action, out=None):
        """(fixed_encoder.zs(state), fixed_encoder.zsa(zs, action)), one launch
        (:248-249); out: a (zs, zsa) pair of [B, Z] fp32 buffers to write."""
        self.refresh("fixed_encoder")
        s, a = state.contiguous(), action.contiguous()
        B = s.shape[0]
        Z = self.L.hp.zs_dim
        if out is not None:
            zs, zsa = out
        else:
            zs = torch.empty((B, Z), dtype=torch.float32, device=s.device)
            zsa = torch.empty((B, Z), dtype=torch.float32, device=s.device)
        nat.check(nat.lib().td7f_fixed(self.prec, self.act, self.nets["fixed_encoder"].array, nat.ptr(s), nat.ptr(a),
                                       B, nat.ptr(zs), nat.ptr(zsa), nat.stream_ptr(s.device)), "td7f_fixed")
        return zs, zsa


class XTBuffers:
    """The transposed weight-gradient operands of one Linear in the operand
    type (include/exo_amd.h td7f_xt)."""

    def __init__(self, N, K, B, ld, dev, prec=1):
        r64 = lambda n: -(-n // 64) * 64  # noqa: E731
        self.N, self.K = N, K
        self.x = torch.zeros((r64(K), ld), dtype=_etype(prec), device=dev)
        self.dp = torch.zeros((r64(N), ld), dtype=_etype(prec), device=dev)
        self.part = torch.zeros((-(-B // 16), N), dtype=torch.float32, device=dev)
        self.c = nat.TD7FXT(self.x.data_ptr(), self.dp.data_ptr(), self.part.data_ptr())


def _grad_views(opt):
    """Persistent gradient tensors of a FlatAdam's parameters: views of one flat
    buffer in parameter order (the fused weight-gradient launch writes them;
    the optimiser step and the data-parallel all-reduce read them)."""
    g = torch.zeros_like(opt.flat)
    off = 0
    for p in opt._params():
        n = p.numel()
        p.grad = g[off:off + n].view_as(p)
        off += n
    return g


class FusedTrain:
    """The gradient passes of one TD7 update as fused launches (csrc/td7_fused_train.hip)
    for a batch of B rows: buffers are allocated on the first call (outside graph capture)."""

    def __init__(self, nets, B):
        self.nets, self.L, self.B = nets, nets.L, B
        L, dev = self.L, nets.dev
        hp = L.hp
        # row stride of the transposed operands = the weight-gradient reduction
        # length: the batch padded to 256 rows (zero columns; td7f_wgrad's k-loop)
        self.ld = -(-B // 256) * 256
        Z, He, Hc, Ha = hp.zs_dim, hp.enc_hdim, hp.critic_hdim, hp.actor_hdim
        A = L.actor.l3.out_features
        S = L.actor.l0.in_features
        self.S, self.A = S, A
        f32 = dict(dtype=torch.float32, device=dev)
        p = nets.prec
        self.xt_enc = [XTBuffers(pl.N, pl.K, B, self.ld, dev, p) for pl in nets.nets["encoder"].layers]
        self.xt_critic = [XTBuffers(pl.N, pl.K, B, self.ld, dev, p) for pl in nets.nets["critic"].layers]
        self.xt_actor = [XTBuffers(pl.N, pl.K, B, self.ld, dev, p) for pl in nets.nets["actor"].layers]
        self.y_enc = [torch.empty((B, He), **f32) for _ in range(4)]
        self.y_critic = [torch.empty((2, B, Hc), **f32) for _ in range(2)]
        self.td = torch.zeros((B, 2), **f32)
        self.q = torch.zeros((B, 2), **f32)
        # the critic pass split in two launches (critic(phase=1 / 2)): the
        # forward's state for the backward -- Q, q0's pre-norm output, row means
        bp = -(-B // 16) * 16
        self.crit_q = torch.zeros((2, bp), **f32)
        self.crit_h0 = torch.zeros((2, bp, Hc), **f32)
        self.crit_mean = torch.zeros((2, bp), **f32)
        self.prio = torch.zeros((B,), **f32)
        self.act_out = torch.zeros((B, A), **f32)
        self.zsa_out = torch.zeros((B, Z), **f32)
        self.h0 = torch.zeros((B, Ha), **f32)
        self.mean0 = torch.zeros((B,), **f32)
        self.ya = [torch.zeros((B, Ha), **f32) for _ in range(2)]
        self.yz = [torch.zeros((B, He), **f32) for _ in range(2)]
        self.yc = [torch.zeros((2, B, Hc), **f32) for _ in range(2)]
        self.da = torch.zeros((2, B, A), **f32)
        self.dzsa = torch.zeros((2, B, Z), **f32)
        # offline (TD3+BC): sum |Q| per (head, row tile), actor(1) -> actor(2)
        self.qabs = torch.zeros((2, -(-B // 16)), **f32)
        P = ctypes.c_void_p
        self.actor_bufs = nat.TD7FActorBufs(self.act_out.data_ptr(), self.zsa_out.data_ptr(), self.h0.data_ptr(),
                                            self.mean0.data_ptr(), (P * 2)(*[t.data_ptr() for t in self.ya]),
                                            (P * 2)(*[t.data_ptr() for t in self.yz]),
                                            (P * 2)(*[t.data_ptr() for t in self.yc]), self.da.data_ptr(),
                                            self.dzsa.data_ptr())
        self.enc_grad = _grad_views(L.encoder_optimizer)
        self.critic_grad = _grad_views(L.critic_optimizer)
        self.actor_grad = _grad_views(L.actor_optimizer)
        # weight-gradient jobs: [layer] (encoder), [layer][head] (critic), [layer] (actor)
        rt = -(-B // 16)
        enc_p = list(L.encoder.parameters())
        jobs = []
        for i, xb in enumerate(self.xt_enc):
            jobs.append(self._job(xb, enc_p[2 * i].grad, enc_p[2 * i + 1].grad, rt))
        for k in range(4):
            gw, gb = getattr(L.critic, f"w{k}").grad, getattr(L.critic, f"b{k}").grad
            for h in range(2):
                jobs.append(self._job(self.xt_critic[2 * k + h], gw[h], gb[h], rt))
        self.jobs_ec = (nat.TD7FWgJob * len(jobs))(*jobs)
        ne = len(self.xt_enc)
        self.jobs_e = (nat.TD7FWgJob * ne)(*jobs[:ne])
        self.jobs_c = (nat.TD7FWgJob * (len(jobs) - ne))(*jobs[ne:])
        # td7f_wgrad_adam: where each job's layer sits in its optimiser (None
        # when the jobs do not cover every parameter of that optimiser)
        self.adam_e = self._adam_descs(L.encoder_optimizer, nets.nets["encoder"].layers)
        self.adam_c = self._adam_descs(L.critic_optimizer, nets.nets["critic"].layers)
        self.adam_a = self._adam_descs(L.actor_optimizer, nets.nets["actor"].layers)
        act_p = list(L.actor.parameters())
        ajobs = [self._job(xb, act_p[2 * i].grad, act_p[2 * i + 1].grad, rt) for i, xb in enumerate(self.xt_actor)]
        self.jobs_a = (nat.TD7FWgJob * len(ajobs))(*ajobs)
        self.ptrs_y_enc = (P * 4)(*[t.data_ptr() for t in self.y_enc])
        # the encoder pass with zs(s') on its own workgroup row (r04, EXO_ENC_SPLIT=1).
        # Off by default: alone the split pass is shorter, but inside the training
        # iteration its extra 64 workgroups take CUs from the concurrent target /
        # fixed passes on the critical chain (0.320 vs 0.299 ms per iteration,
        # profiles/r04b_raw/bench_ab_*.log)
        self.enc_split = os.environ.get("EXO_ENC_SPLIT", "0") == "1"
        self.enc_nz = torch.zeros((rt * 16, Z), **f32)
        self.enc_flag = torch.zeros((rt,), dtype=torch.int32, device=dev)

    @staticmethod
    def _adam_descs(opt, layers):
        flat = getattr(opt, "flat", None)
        if flat is None:
            return None
        base, descs, covered = flat.data_ptr(), [], 0
        for pl in layers:
            w, b = pl.weight, pl.bias
            descs.append(nat.TD7FWgAdam(0, (w.data_ptr() - base) // 4, (b.data_ptr() - base) // 4, pl.wf.data_ptr(),
                                        pl.wb.data_ptr() if pl.wb is not None else None, pl.ksf, pl.ksb))
            covered += w.numel() + b.numel()
        return (nat.TD7FWgAdam * len(descs))(*descs) if covered == flat.numel() else None

    def fuses_adam(self):
        """The weight-gradient launches can carry the optimiser steps (every
        parameter of the encoder / critic / actor optimisers is one of their layers)."""
        return all(d is not None for d in (self.adam_e, self.adam_c, self.adam_a))

    def _wgrad(self, jobs, descs, opt, adam, td=None, prio=None, B=0):
        fz, hp = self.nets, self.L.hp
        if adam and descs is None:
            raise RuntimeError("td7f_wgrad_adam: the layers do not cover the optimiser's parameters")
        st = nat.stream_ptr(fz.dev)
        alpha, minp = (float(hp.alpha), float(hp.min_priority)) if prio is not None else (0.0, 0.0)
        if not adam:
            nat.check(nat.lib().td7f_wgrad(fz.prec, len(jobs), jobs, self.ld, self.ld, td, prio, B, alpha, minp, st),
                      "td7f_wgrad")
            return
        g = opt.param_groups[0]
        P1 = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
        F1 = lambda x: (ctypes.c_float * 1)(float(x))  # noqa: E731
        nat.check(nat.lib().td7f_wgrad_adam(fz.prec, len(jobs), jobs, self.ld, self.ld, td, prio, B, alpha, minp, 1,
                                            P1(opt.flat), P1(opt.m), P1(opt.v), P1(opt._step), F1(g["lr"]),
                                            F1(g["betas"][0]), F1(g["betas"][1]), F1(g["eps"]),
                                            F1(g["weight_decay"]), descs, nat.ptr(opt._ticket), st), "td7f_wgrad_adam")

    @staticmethod
    def _job(xb, gw, gb, rt):
        assert gw.is_contiguous() and gb.is_contiguous()
        return nat.TD7FWgJob(xb.dp.data_ptr(), xb.x.data_ptr(), xb.part.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                             xb.N, xb.K, rt)

    @staticmethod
    def _xts(bufs):
        return (nat.TD7FXT * len(bufs))(*[b.c for b in bufs])

    def encoder(self, state, action, next_state):
        fz = self.nets
        fz.refresh("encoder")
        nz, fl = (self.enc_nz, self.enc_flag) if self.enc_split else (None, None)
        nat.check(nat.lib().td7f_encoder(fz.prec, fz.act, fz.nets["encoder"].array, nat.ptr(state), nat.ptr(action),
                                         nat.ptr(next_state), self.B, self.ptrs_y_enc, self._xts(self.xt_enc), self.ld,
                                         nat.ptr(nz), nat.ptr(fl), nat.stream_ptr(state.device)), "td7f_encoder")

    def critic(self, state, action, zs, zsa, qt, reward, not_done, phase=0):
        """td7f_critic_phase: 0 the whole critic pass; 1 its forward alone (needs
        no qt: it runs beside the target chain); 2 the loss and the backward
        from phase 1's stored state -- phases 1 + 2 == phase 0 bit for bit."""
        fz, L = self.nets, self.L
        if phase != 2:
            fz.refresh("critic")
        nat.check(nat.lib().td7f_critic_phase(
            int(phase), fz.prec, fz.act, fz.nets["critic"].array, nat.ptr(state), nat.ptr(action), nat.ptr(zs),
            nat.ptr(zsa), nat.ptr(qt), nat.ptr(reward), nat.ptr(not_done), float(L.hp.discount),
            nat.ptr(L.min_target), nat.ptr(L.max_target), nat.ptr(L.max), nat.ptr(L.min), self.B, self.S, self.A,
            nat.ptr(self.td), nat.ptr(self.q), nat.ptr(self.y_critic[0]), nat.ptr(self.y_critic[1]),
            self._xts(self.xt_critic), self.ld, nat.ptr(self.crit_q), nat.ptr(self.crit_h0), nat.ptr(self.crit_mean),
            nat.stream_ptr(state.device)), "td7f_critic_phase")

    def wgrad_encoder_critic(self):
        """Every encoder and critic weight/bias gradient (one launch) and the LAP priorities."""
        fz, hp = self.nets, self.L.hp
        nat.check(nat.lib().td7f_wgrad(fz.prec, len(self.jobs_ec), self.jobs_ec, self.ld, self.ld, nat.ptr(self.td),
                                       nat.ptr(self.prio), self.B, float(hp.alpha), float(hp.min_priority),
                                       nat.stream_ptr(fz.dev)), "td7f_wgrad")
        return self.prio

    def wgrad_encoder(self, adam=False):
        """The encoder's weight/bias gradients alone (its branch of the update);
        adam: with the encoder's optimiser step and repack (td7f_wgrad_adam)."""
        L = self.L
        self._wgrad(self.jobs_e, self.adam_e, L.encoder_optimizer, adam)

    def wgrad_critic(self, adam=False):
        """The critic's weight/bias gradients and the LAP priorities; adam: with
        the critic's optimiser step and repack."""
        L = self.L
        self._wgrad(self.jobs_c, self.adam_c, L.critic_optimizer, adam, nat.ptr(self.td),
                    nat.ptr(self.prio), self.B)
        return self.prio

    def actor(self, phase, state, zs, action=None, lmbda=0.0):
        """td7f_actor; action given: td7f_actor_bc, the offline update's TD3+BC
        term lmbda |Q|.mean() mse(actor, action) with it (phase 1 leaves the
        |Q| partials in self.qabs, phase 2 reads them and the batch actions)."""
        fz = self.nets
        fz.refresh("actor", "fixed_encoder", "critic")
        if action is not None:
            nat.check(nat.lib().td7f_actor_bc(fz.prec, phase, fz.act, fz.nets["actor"].array,
                                              fz.nets["fixed_encoder"].array, fz.nets["critic"].array, nat.ptr(state),
                                              nat.ptr(zs), nat.ptr(action), float(lmbda), nat.ptr(self.qabs), self.B,
                                              ctypes.byref(self.actor_bufs), self._xts(self.xt_actor), self.ld,
                                              nat.stream_ptr(state.device)), f"td7f_actor_bc[{phase}]")
            return
        nat.check(nat.lib().td7f_actor(fz.prec, phase, fz.act, fz.nets["actor"].array, fz.nets["fixed_encoder"].array,
                                       fz.nets["critic"].array, nat.ptr(state), nat.ptr(zs), self.B,
                                       ctypes.byref(self.actor_bufs), self._xts(self.xt_actor), self.ld,
                                       nat.stream_ptr(state.device)), f"td7f_actor[{phase}]")

    def wgrad_actor(self, adam=False):
        self._wgrad(self.jobs_a, self.adam_a, self.L.actor_optimizer, adam)


# ------------------------------------------------------------------ many policies, one launch
def multi_tiles(seg, rows=16):
    """The tile table of td7f_select_multi (include/exo_amd.h): policy p owns
    the rows [seg[p], seg[p+1]); each segment is cut into ceil(len / rows)
    tiles from its first row, the last one ragged, so no tile straddles two
    segments.  seg: non-decreasing integers, seg[0] == 0.  Returns int32
    [ntiles, 3] = (policy, row0, row_end); empty segments give no tiles."""
    s = np.asarray(seg)
    if s.ndim != 1 or s.size < 2 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("multi_tiles: seg must be a 1-D integer array of npol + 1 entries")
    s = s.astype(np.int64)
    if s[0] != 0 or np.any(np.diff(s) < 0) or s[-1] >= 2 ** 31 or int(rows) <= 0:
        raise ValueError("multi_tiles: seg must start at 0, not decrease and stay below 2^31")
    rows = int(rows)
    cnt = -(-np.diff(s) // rows)
    pol = np.repeat(np.arange(s.size - 1, dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt  # index of each policy's first tile
    row0 = s[:-1][pol] + (np.arange(pol.size, dtype=np.int64) - first[pol]) * rows
    return np.stack([pol, row0, np.minimum(row0 + rows, s[1:][pol])], axis=1).astype(np.int32).reshape(-1, 3)


def _select_multi_call(fn, prec, act, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, middle, out, scale,
                       npol):
    """fn: one of the td7f_select_multi* entry points, which share their first
    eleven and last three arguments; middle: the ones between."""
    npol = len(seg) - 1 if npol is None else npol
    cseg = (ctypes.c_int32 * len(seg))(*[int(v) for v in seg])
    return fn(prec, act, npol, enc, actor, nat.ptr(policies_dev), cseg, nat.ptr(tiles_dev), int(ntiles), nat.ptr(obs),
              int(n), *middle, nat.ptr(out), float(scale), nat.stream_ptr(obs.device))


def select_multi_raw(prec, act, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, noise, out, scale,
                     npol=None):
    """td7f_select_multi as it stands in the C ABI; returns its status code.
    enc / actor: TD7FLin arrays of 3 / 4 entries per policy; seg: a python
    sequence of npol + 1 ints; noise: a TD7FNoise or None (deterministic)."""
    return _select_multi_call(nat.lib().td7f_select_multi, prec, act, enc, actor, policies_dev, seg, tiles_dev,
                              ntiles, obs, n, (ctypes.byref(noise) if noise is not None else None,), out, scale, npol)


def per_policy(value, K, name, owner="MultiNoise"):
    """A scalar or a length-K sequence as a list of K floats, none negative
    (sigma, sigma_dec, clip of K behaviour policies)."""
    v = np.asarray(value, dtype=np.float64)
    if v.ndim == 0:
        v = np.full((K,), float(v))
    if v.shape != (K,):
        raise ValueError(f"{owner}: {name} must be a scalar or hold {K} values")
    if not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError(f"{owner}: {name} must be finite and >= 0")
    return [float(x) for x in v]


# The tags of the Philox streams a MultiNoise owns: policy p draws from tag
# MULTI_NOISE_TAG0 + p.  The project's other consumers use small tags (the
# learner's exploration stream is 2, the replay's sampler and the target noise
# sit next to it), so no policy shares a stream with them or with another
# policy of the set.
MULTI_NOISE_TAG0 = 0x4D4E0000
# ... and the stream a learner's own PinkNoise draws from (PinkNoise.for_learner):
# outside the MULTI_NOISE_TAG0 + p and + 0x8000 + p ranges and the small tags
LEARNER_PINK_TAG = 0x504B0000


class _OnePolicy:
    """What PinkNoise and MultiNoise read of a PolicySet, for one learner with
    no set: one policy whose rows are all n envs."""

    def __init__(self, dev, A, n):
        self.dev, self.A, self.n = dev, A, int(n)
        self._seg_dev = torch.tensor([0, self.n], dtype=torch.int32).to(dev)

    def __len__(self):
        return 1

    def _key(self, seg):
        key = tuple(int(v) for v in seg)
        if key != (0, self.n):
            raise ValueError(f"PinkNoise.for_learner: seg is [0, {self.n}]")
        return key

    def tiles(self, seg):
        return self._key(seg), None, -(-self.n // 16)

    def seg_dev(self, seg):
        self._key(seg)
        return self._seg_dev


class MultiNoise:
    """One exploration-noise state per policy of a PolicySet, for
    PolicySet.act(noise=...) (td7f_select_multi_noise): policy p's rows get
    clamp(a + c_p(z * sigma_p), -1, 1) * scale with z from policy p's own
    Philox stream, element (row - seg[p]) * A + column -- TD7_multi_agent.py
    :192-209 per policy.  After a launch every policy that had rows has
    sigma_p -= sigma_dec_p and its call counter advanced.

    sigma, sigma_dec, clip: scalars or length-K sequences.  By default the
    object owns one ops.DeviceRNG per policy (tags: tags, default
    MULTI_NOISE_TAG0 + p, all distinct) and one fp32 [K] sigma tensor.
    states=[(rng, sigma_tensor), ...] binds existing state instead -- e.g. an
    agent's learner._explore_rng / exploration_noise_t -- and `sigma` is then
    ignored (None).  The device table is built once; it holds pointers, so the
    bound tensors must stay alive and in place."""

    def __init__(self, policy_set, sigma, sigma_dec=0.0, clip=0.0, tags=None, states=None):
        K = len(policy_set)
        self.K = K
        self.dev = policy_set.dev
        self.sigma_dec = per_policy(sigma_dec, K, "sigma_dec")
        self.clip = per_policy(clip, K, "clip")
        if states is not None:
            states = list(states)
            if len(states) != K:
                raise ValueError(f"MultiNoise: states must hold {K} (rng, sigma) pairs")
            self.rngs = [s[0] for s in states]
            self.sigmas = [s[1] for s in states]
            for t in self.sigmas:
                if t.dtype != torch.float32 or t.numel() != 1 or t.device != self.dev:
                    raise ValueError(f"MultiNoise: a bound sigma must be one float32 on {self.dev}")
            self.sigma = None
            self.owns_state = False
        else:
            if tags is None:
                tags = [MULTI_NOISE_TAG0 + p for p in range(K)]
            tags = [int(t) for t in tags]
            if len(tags) != K or len(set(t & 0xFFFFFFFF for t in tags)) != K:
                raise ValueError(f"MultiNoise: tags must hold {K} distinct values")
            self.sigma0 = per_policy(sigma, K, "sigma")
            self.rngs = [ops.DeviceRNG(self.dev, t) for t in tags]
            self.sigma = torch.tensor(self.sigma0, dtype=torch.float32, device=self.dev)
            self.sigmas = [self.sigma[p:p + 1] for p in range(K)]
            self.owns_state = True
        # one ticket word for the launch (zero between launches)
        self.ticket = torch.zeros((2,), dtype=torch.int32, device=self.dev)
        per = (TD7FNoise * K)(*[TD7FNoise(r.seed, r.tag, 0, r.counter_ptr, None, s.data_ptr(), d, c, 1.0, 0, None,
                                          None)
                                for r, s, d, c in zip(self.rngs, self.sigmas, self.sigma_dec, self.clip)])
        self.rows = (nat.TD7FNoiseRow * K)()
        nat.check(nat.lib().td7f_multi_noise_table(K, per, self.rows), "td7f_multi_noise_table")
        self.table = torch.frombuffer(bytearray(bytes(self.rows)), dtype=torch.uint8).to(self.dev)

    def sigma_now(self):
        """every policy's sigma (one host read per bound tensor, or one)"""
        if self.sigma is not None:
            return [float(v) for v in self.sigma.cpu()]
        return [float(t) for t in self.sigmas]

    def counters(self):
        """every policy's call counter (host reads)"""
        return [int(r.state[0]) for r in self.rngs]


def select_multi_noise_raw(prec, act, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, rows, noise_dev,
                           seg_dev, ticket, z, out, scale, npol=None):
    """td7f_select_multi_noise as it stands in the C ABI; returns its status
    code.  rows: the host TD7FNoiseRow array (or None), noise_dev / seg_dev /
    ticket / z: device tensors (or None)."""
    middle = (rows, nat.ptr(noise_dev), nat.ptr(seg_dev), nat.ptr(ticket), nat.ptr(z))
    return _select_multi_call(nat.lib().td7f_select_multi_noise, prec, act, enc, actor, policies_dev, seg, tiles_dev,
                              ntiles, obs, n, middle, out, scale, npol)


class PinkNoise:
    """One coloured (power-law, exponent beta) noise sequence per env of a
    PolicySet layout, for PolicySet.act(noise=...) (td7f_select_multi_seq) --
    TD7_multi_agent_Pink_noise.py:203-228 per env, with asynchronous episodes:
    env r of policy p owns the row seq[r] ([Lmax, A]; its first lengths[r]
    steps are used), peak-normalised and scaled by sigma_p as it stood when the
    env's episode began; step t[r] of its episode adds seq[r, t[r]].
    advance(stepped, done) after every env step counts the steps and
    regenerates the rows of finished episodes (td7f_pink_advance), all on the
    device: no host read, so a step with it can be captured in a graph.

    seg: the layout PolicySet.act is called with; lengths: every env's
    sequence length (VecExoskeletonEnv.lengths_host).  sigma, sigma_dec, clip,
    tags as MultiNoise, whose device table, sigma tensor and DeviceRNGs this
    object holds (default tags MULTI_NOISE_TAG0 + 0x8000 + p: distinct from a
    MultiNoise of the same set).  Row r draws from its policy's stream at call
    epi[r], the index of its episode; the streams' call counters stay 0."""

    def __init__(self, policy_set, seg, lengths, sigma, sigma_dec=0.0, clip=0.0, beta=1.0, tags=None, states=None):
        from . import pink
        K = len(policy_set)
        if tags is None:
            tags = [MULTI_NOISE_TAG0 + 0x8000 + p for p in range(K)]
        # states: MultiNoise's [(rng, sigma tensor), ...] bound instead of owned (for_learner)
        self.multi = MultiNoise(policy_set, sigma, sigma_dec, clip, tags=tags, states=states)
        self.K, self.dev, self.A = K, policy_set.dev, policy_set.A
        self.table, self.rows, self.ticket = self.multi.table, self.multi.rows, self.multi.ticket
        self.sigma, self.rngs = self.multi.sigma, self.multi.rngs
        self.beta = float(beta)
        self.seg, _, _ = policy_set.tiles(seg)
        self.seg_dev = policy_set.seg_dev(seg)
        self.n = n = self.seg[-1]
        lengths = np.asarray(lengths)
        if lengths.shape != (n,):
            raise ValueError(f"PinkNoise: lengths must hold one value for each of the {n} envs")
        len_cls, cls_len, cls_scale, cls_norm = pink.length_classes(lengths, self.beta)
        self.lengths_host = lengths.astype(np.int64)
        self.Lmax = int(cls_len[-1])
        self.nf_max = self.Lmax // 2 + 1
        self.cls_len_host = (ctypes.c_int32 * len(cls_len))(*[int(v) for v in cls_len])
        self._cseg = (ctypes.c_int32 * len(self.seg))(*self.seg)
        d = self.dev
        self.len_cls = torch.as_tensor(len_cls).to(d)
        self.cls_len = torch.as_tensor(cls_len).to(d)
        self.cls_scale = torch.as_tensor(cls_scale).contiguous().to(d)
        self.cls_norm = torch.as_tensor(cls_norm).to(d)
        self.seq = torch.zeros((n, self.Lmax, self.A), dtype=torch.float32, device=d)
        self.t = torch.zeros((n,), dtype=torch.int32, device=d)
        # the index of the episode whose sequence a row holds: the fill below is episode 0
        self.epi = torch.full((n,), -1, dtype=torch.int32, device=d)
        ones = torch.ones((n,), dtype=torch.bool, device=d)
        self.advance(ones, ones)

    @classmethod
    def for_learner(cls, fused_nets, lengths, clip=0.0, beta=None, tag=LEARNER_PINK_TAG, sigma=None):
        """The sequences of one learner's envs, for FusedNets.select(pink=...)
        (td7f_select_seq) -- no PolicySet: one policy, seg = [0, n].  sigma is
        the learner's own exploration_noise_t, bound (sigma=: another float32
        device scalar to bind instead), so Gaussian and pink calls move one
        schedule; sigma_dec its action_noise_decrease (one decrement per
        call, :225); beta defaults to hp.beta.  The rows draw from a DeviceRNG
        of this object's own (tag): they draw at call index epi[r], which in
        the learner's exploration stream would be a Gaussian call's index."""
        L = fused_nets.L
        n = len(lengths)
        layout = _OnePolicy(fused_nets.dev, L.actor.l3.out_features, n)
        rng = ops.DeviceRNG(fused_nets.dev, int(tag))
        sig = L.exploration_noise_t if sigma is None else sigma
        return cls(layout, [0, n], lengths, None, L.action_noise_decrease, clip,
                   beta=L.hp.beta if beta is None else beta, states=[(rng, sig)])

    def noise(self, scale=1.0):
        """policy 0's state as the td7f_noise of a td7f_select_seq call: sigma,
        sigma_dec, clip, this object's ticket word (no Philox state is used)"""
        r = self.rngs[0]
        return TD7FNoise(r.seed, r.tag, 0, r.counter_ptr, self.ticket.data_ptr(), self.multi.sigmas[0].data_ptr(),
                         self.multi.sigma_dec[0], self.multi.clip[0], float(scale), 0, None, None)

    def sigma_now(self):
        return self.multi.sigma_now()

    def _mask(self, m, name):
        if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != (self.n,) or m.device != self.dev \
                or not m.is_contiguous():
            raise ValueError(f"PinkNoise.advance: {name} must be contiguous bool / uint8 [{self.n}] on {self.dev}")
        return m

    def _spec(self, s, name):
        shape = (self.n, self.A, self.nf_max, 2)
        if s is not None and (tuple(s.shape) != shape or s.dtype != torch.float32 or s.device != self.dev
                              or not s.is_contiguous()):
            raise ValueError(f"PinkNoise.advance: {name} must be contiguous float32 {shape} on {self.dev}")
        return s

    @torch.no_grad()
    def advance(self, stepped, done, spectrum=None, spec_out=None, peak_out=None):
        """One td7f_pink_advance launch: t += 1 where stepped; where done, t =
        0, epi += 1 and the env's sequence regenerated.  spectrum (float32 [n,
        A, nf_max, 2] = (sr, si), already scaled) replaces the Philox draws;
        spec_out (same shape) / peak_out (float32 [n]) receive the regenerated
        rows' scaled spectra before the masking and their peaks."""
        self._mask(stepped, "stepped")
        self._mask(done, "done")
        self._spec(spectrum, "spectrum")
        self._spec(spec_out, "spec_out")
        if peak_out is not None and (tuple(peak_out.shape) != (self.n,) or peak_out.dtype != torch.float32
                                     or peak_out.device != self.dev or not peak_out.is_contiguous()):
            raise ValueError(f"PinkNoise.advance: peak_out must be contiguous float32 [{self.n}] on {self.dev}")
        nat.check(nat.lib().td7f_pink_advance(self.K, self._cseg, self.n, self.A, self.Lmax, len(self.cls_len_host),
                                              self.cls_len_host, nat.ptr(stepped), nat.ptr(done), nat.ptr(self.t),
                                              nat.ptr(self.epi), nat.ptr(self.seq), nat.ptr(self.len_cls),
                                              nat.ptr(self.cls_len), nat.ptr(self.cls_norm), nat.ptr(self.cls_scale),
                                              self.rows, nat.ptr(self.table), nat.ptr(self.seg_dev),
                                              nat.ptr(spectrum), nat.ptr(spec_out), nat.ptr(peak_out),
                                              nat.stream_ptr(self.dev)), "td7f_pink_advance")


def select_multi_seq_raw(prec, act, enc, actor, policies_dev, seg, tiles_dev, ntiles, obs, n, rows, noise_dev,
                         seg_dev, ticket, seq, t, Lmax, out, scale, npol=None):
    """td7f_select_multi_seq as it stands in the C ABI; returns its status code."""
    middle = (rows, nat.ptr(noise_dev), nat.ptr(seg_dev), nat.ptr(ticket), nat.ptr(seq), nat.ptr(t), int(Lmax))
    return _select_multi_call(nat.lib().td7f_select_multi_seq, prec, act, enc, actor, policies_dev, seg, tiles_dev,
                              ntiles, obs, n, middle, out, scale, npol)


class PolicySet:
    """K policies -- (actor, fixed encoder) module pairs of one shape -- packed
    for td7f_select_multi: one launch in which policy p acts on the rows
    [seg[p], seg[p+1]) of the observations (TD7_multi_agent.py:192-209 /
    TD7_multi_agent_Pink_noise.py:212-214 per policy).  The set owns packed
    forward-only copies of the modules' weights (PackedNet) and the device
    policy table (pointers and shapes: refresh() repacks in place and keeps
    it); it reads the modules and changes nothing of theirs."""

    def __init__(self, policies, precision, device, activations=None):
        from .td7 import Hyperparameters
        if precision not in PREC:
            raise ValueError(f"PolicySet: precision must be one of {sorted(PREC)}")
        policies = list(policies)
        if not policies:
            raise ValueError("PolicySet: no policies")
        self.prec = PREC[precision]
        self.precision = precision
        self.dev = nat.require_gpu(device)
        if activations is None:
            hp = Hyperparameters()
            activations = (hp.enc_activ, hp.actor_activ)
        codes = [ops.act_code(f) for f in activations]
        if any(c is None or c == ops.ACT_CODES["tanh"] for c in codes):
            raise ValueError("PolicySet: activations must be relu or elu")
        self.act_codes = (ctypes.c_int32 * 3)(codes[0], codes[1], 0)
        self.policies = policies
        self.nets = []
        for actor, enc in policies:
            layers = encoder_layers(enc)[:3] + actor_layers(actor)
            if any(w.device != self.dev or w.dtype != torch.float32 for w, _ in layers):
                raise ValueError(f"PolicySet: the modules must hold fp32 weights on {self.dev}")
            self.nets.append(PackedNet(layers, self.prec))
        shape0 = [(pl.N, pl.K) for pl in self.nets[0].layers]
        for k, net in enumerate(self.nets):
            if [(pl.N, pl.K) for pl in net.layers] != shape0:
                raise ValueError(f"PolicySet: policy {k} has another shape than policy 0 (one LDS plan serves the launch)")
        self.S, self.A = self.nets[0].layers[0].K, self.nets[0].layers[6].N
        self.enc = _lin_array([pl for net in self.nets for pl in net.layers[:3]])
        self.actor = _lin_array([pl for net in self.nets for pl in net.layers[3:]])
        # the device policy table, td7f_lin [K][7], from the arrays the launch validates
        host = (TD7FLin * (7 * len(self.nets)))()
        nat.check(nat.lib().td7f_multi_policy_table(len(self.nets), self.enc, self.actor, host),
                  "td7f_multi_policy_table")
        self.table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(self.dev)
        self._tiles = {}
        self.pack()
        self._probe()

    @classmethod
    def from_agents(cls, agents, use_checkpoint=True, precision=None, device=None):
        """The agents' checkpoint policies (checkpoint_actor / checkpoint_encoder:
        what TD7 reports) or, use_checkpoint=False, their live ones (actor /
        fixed_encoder)."""
        agents = list(agents)
        L0 = agents[0].learner
        pairs = [(a.learner.checkpoint_actor, a.learner.checkpoint_encoder) if use_checkpoint
                 else (a.learner.actor, a.learner.fixed_encoder) for a in agents]
        return cls(pairs, precision or L0.precision, device or L0.device, (L0.hp.enc_activ, L0.hp.actor_activ))

    def __len__(self):
        return len(self.nets)

    def _probe(self):
        """the launch's arguments and LDS plan checked once (td7f_probe)"""
        n = 16 * len(self)
        seg = [16 * k for k in range(len(self) + 1)]
        obs = torch.zeros((n, self.S), dtype=torch.float32, device=self.dev)
        lib = nat.lib()
        lib.td7f_probe(1)
        try:
            try:
                self.act(obs, seg)
                self.act(obs, seg, noise=MultiNoise(self, 0.0))
            except RuntimeError as e:
                raise PlanError(f"td7f_select_multi cannot run this policy shape: {e}") from e
        finally:
            lib.td7f_probe(0)

    def pack(self, k=None):
        """td7f_pack of policy k's (None: every policy's) weights, TD7F_MAX_PACK jobs per launch."""
        nets = self.nets if k is None else [self.nets[k]]
        jobs = [pl.job() for net in nets for pl in net.layers]
        st = nat.stream_ptr(self.dev)
        for i in range(0, len(jobs), MAX_PACK):
            part = jobs[i:i + MAX_PACK]
            nat.check(nat.lib().td7f_pack(self.prec, len(part), (TD7FPackJob * len(part))(*part), st), "td7f_pack")
        for net in nets:
            net._ver = net._versions()

    def refresh(self, k=None):
        """Repack policy k (None: every policy) when its master weights changed
        through torch since its last pack (version counters, PackedNet.refresh);
        weights written by a HIP kernel need pack()."""
        ks = range(len(self)) if k is None else [k]
        for j in ks:
            if self.nets[j]._versions() != self.nets[j]._ver:
                self.pack(j)

    def tiles(self, seg):
        """(seg as a tuple, device tile table, ntiles) for seg; built once per
        seg -- a new one needs an allocation and a copy, so not inside a capture."""
        key = tuple(int(v) for v in seg)
        hit = self._tiles.get(key)
        if hit is None:
            if len(key) != len(self) + 1:
                raise ValueError(f"PolicySet: seg needs {len(self) + 1} entries")
            if self.dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("PolicySet.act: call once eagerly with this seg before graph capture")
            t = multi_tiles(np.asarray(key, dtype=np.int64))
            # (an empty table still needs an address)
            dev = torch.as_tensor(t if len(t) else np.zeros((1, 3), np.int32)).to(self.dev)
            # the device copy of seg td7f_select_multi_noise reads, built with the tile table
            hit = self._tiles[key] = (dev, len(t), torch.tensor(key, dtype=torch.int32).to(self.dev))
        return key, hit[0], hit[1]

    def seg_dev(self, seg):
        """the device copy of seg (int32 [K + 1]) cached with its tile table"""
        key, _, _ = self.tiles(seg)
        return self._tiles[key][2]

    @torch.no_grad()
    def act(self, obs, seg, out=None, scale=1.0, noise=None, z=None):
        """One td7f_select_multi launch: out[r] = policy p's action for obs[r],
        seg[p] <= r < seg[p+1].  noise None: deterministic, clamp(tanh(.), -1,
        1) * scale, no noise state touched; a TD7FNoise (FusedNets._noise):
        that one exploration-noise state for the whole launch (its own scale
        applies); a MultiNoise: every policy its own state
        (td7f_select_multi_noise), times `scale`, and z (float32 [n, A]
        standard normals) then replaces the Philox draws and leaves the
        counters alone; a PinkNoise: every env column t of its own coloured
        sequence (td7f_select_multi_seq), times `scale`.  Repack changed
        weights with refresh() first."""
        key, tiles, nt = self.tiles(seg)
        obs = obs.contiguous()
        n = obs.shape[0]
        if obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != self.S:
            raise ValueError(f"PolicySet.act: obs must be float32 [n, {self.S}]")
        if out is None:
            out = torch.empty((n, self.A), dtype=torch.float32, device=obs.device)
        elif tuple(out.shape) != (n, self.A) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"PolicySet.act: out must be contiguous float32 {(n, self.A)}")
        if isinstance(noise, MultiNoise):
            if noise.K != len(self):
                raise ValueError(f"PolicySet.act: the MultiNoise holds {noise.K} policies, the set {len(self)}")
            if z is not None and (tuple(z.shape) != (n, self.A) or z.dtype != torch.float32
                                  or not z.is_contiguous() or z.device != obs.device):
                raise ValueError(f"PolicySet.act: z must be contiguous float32 {(n, self.A)} on {obs.device}")
            nat.check(select_multi_noise_raw(self.prec, self.act_codes, self.enc, self.actor, self.table, key, tiles,
                                             nt, obs, n, noise.rows, noise.table, self._tiles[key][2], noise.ticket,
                                             z, out, scale), "td7f_select_multi_noise")
            return out
        if isinstance(noise, PinkNoise):
            if noise.K != len(self) or noise.seg != key:
                raise ValueError(f"PolicySet.act: the PinkNoise was built for {noise.K} policies and seg "
                                 f"{list(noise.seg)}, not {len(self)} and {list(key)}")
            if z is not None:
                raise ValueError("PolicySet.act: z goes with a MultiNoise")
            nat.check(select_multi_seq_raw(self.prec, self.act_codes, self.enc, self.actor, self.table, key, tiles,
                                           nt, obs, n, noise.rows, noise.table, noise.seg_dev, noise.ticket,
                                           noise.seq, noise.t, noise.Lmax, out, scale), "td7f_select_multi_seq")
            return out
        if z is not None:
            raise ValueError("PolicySet.act: z goes with a MultiNoise")
        nat.check(select_multi_raw(self.prec, self.act_codes, self.enc, self.actor, self.table, key, tiles, nt, obs,
                                   n, noise, out, scale), "td7f_select_multi")
        return out
