"""Helpers of the attribute SCMs: batching and walking a flow's transforms (no dependency beyond torch)."""


def batchify(*tensors, batch_size=128):
    """tuples of aligned slices of ``batch_size`` rows; the last one may be shorter"""
    n = min(len(t) for t in tensors)
    for start in range(0, n, batch_size):
        yield tuple(t[start:start + batch_size] for t in tensors)


def dist_parameters(dist):
    return [p for t in dist.transforms if hasattr(t, "parameters") for p in t.parameters()]


def nf_forward(d, noise):
    """noise -> value through ``d.transforms`` in order"""
    for t in d.transforms:
        noise = t(noise)
    return noise


def nf_inverse(d, obs):
    """value -> noise: the inverses in reverse order"""
    for t in reversed(d.transforms):
        obs = t.inv(obs)
    return obs
