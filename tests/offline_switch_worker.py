"""Child process of tests/test_offline_fused_gpu.py (f): started with
EXO_OFFLINE_FUSED=0, it runs the switch case's two steps and saves the offline
actor gradients (and whether they are views into the fused gradient buffer)."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "a-deep-reinforcement-learning-enabled-soft-exoskeleton-for-parkinson-s-patients_amd")
for p in (HERE, PKG, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main(out):
    from test_fused_train_parity_gpu import _in
    from test_offline_fused_gpu import SWITCH_CASE, actor_grads, forced_steps, offline_learner
    precision, width, B, lmbda = SWITCH_CASE
    L = offline_learner(precision, width, B, lmbda)
    _, b = forced_steps(L, B)
    L.phase_actor_grads(b[0], b[1])
    torch.cuda.synchronize()
    res = {n: g.cpu() for n, g in actor_grads(L).items()}
    res["fused_view"] = torch.tensor(int(_in(L.actor.l0.weight.grad, L.fused.train(B).actor_grad)))
    torch.save(res, out)


if __name__ == "__main__":
    main(sys.argv[1])
