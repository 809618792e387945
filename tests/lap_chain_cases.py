"""Update-index patterns for the sibling-chain tests (tests/test_lap_chain_host.py,
tests/test_lap_update_sample_chain_gpu.py): the collisions the chain must
resolve exactly -- duplicates of one slot, draws below each other's siblings
at every global level, a whole batch inside one 64-leaf block."""
import numpy as np

NTOP = 8192  # csrc/lap.hip TOPN_US: the nodes lap_update_sample keeps in LDS


def global_levels(cap):
    """Levels 1 .. log2(cap) whose nodes lie outside the staged top."""
    levels = cap.bit_length() - 1
    return sum(1 for lv in range(1, levels + 1) if (2 * cap >> lv) > NTOP // 2)


def pattern_names(cap):
    return (["all_equal", "pairs_xor1"] + [f"pair_lv{lv}" for lv in range(max(global_levels(cap), 1))] +
            ["one_block", "ends", "dups"])


def pattern(name, rng, B, size):
    """int32 [B] slots below `size` of one stratum."""
    rnd = lambda: rng.integers(0, size, B).astype(np.int64)  # noqa: E731
    if name == "all_equal":
        idx = np.full(B, rng.integers(0, size), dtype=np.int64)
    elif name == "pairs_xor1":
        idx = rnd()
        idx[1::2] = idx[::2][:idx[1::2].shape[0]] ^ 1
    elif name.startswith("pair_lv"):
        bit = 1 << int(name[7:])
        idx = rnd()
        i = int(rng.integers(0, max(1, size - 2 * bit)))
        idx[:2] = [i, i ^ bit][:B]
        idx[-2:] = [i ^ bit, i][-min(B, 2):]  # and once more, the other way round: later duplicates of both
    elif name == "one_block":
        base = 64 * int(rng.integers(0, max(1, size // 64)))
        idx = base + rng.integers(0, min(64, size), B)
    elif name == "ends":
        idx = rnd()
        idx[:2] = [0, size - 1][:B]
    elif name == "dups":
        idx = rnd()
        idx[1::5] = idx[::5][:idx[1::5].shape[0]]
    else:
        raise KeyError(name)
    return np.minimum(idx, size - 1).astype(np.int32)
