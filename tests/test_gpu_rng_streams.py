"""The device definition of the counter RNG (csrc/ali_rng.h) through the seven launchers that draw from it: bit-equal to
the streams recorded from the kernels as they were before the key schedule moved into that header
(tests/rng_cases.py, tests/golden/rng_streams.npz: the ``dev.*`` entries), the masks bit-equal to the host's
``rng.mask_reference``, and one ``ValueError`` for a malformed counter everywhere."""
import pytest
import torch

import rng_cases as rc
from ali_hip import ops, rng

pytestmark = pytest.mark.gpu


def test_device_streams_match_the_recorded_ones():
    golden = {k: v for k, v in rc.load().items() if k.startswith("dev.")}
    now = rc.device_streams()
    assert golden and set(now) == set(golden)
    for k, v in golden.items():
        assert now[k].dtype == v.dtype and torch.equal(torch.from_numpy(now[k]), torch.from_numpy(v)), k


def test_dropout_mask_is_the_host_reference():
    for _, seed, counter, offset in rc.combos():
        ctr = None if counter is None else torch.full((1,), counter, dtype=torch.int64, device="cuda")
        for B, C in rc.MASK_SHAPES:
            for p in rc.MASK_P:
                got = ops.dropout_mask(seed, offset, p, B, C, "cuda", dev_counter=ctr)
                assert torch.equal(got.cpu(), rng.mask_reference(seed, counter, B, C, p, offset)), (seed, counter, offset, B, C, p)


def test_dropout_mask_multi_is_the_host_reference():
    ends, ps, clog, cpad = rc.multi_layout()
    for seed, counter in rc.KEYS:
        ctr = None if counter is None else torch.full((1,), counter, dtype=torch.int64, device="cuda")
        out = ops.dropout_mask_multi(seed, ctr, ends, ps, clog, cpad, torch.zeros(ends[-1], device="cuda")).cpu()
        lo = draws = 0
        for (B, cl, cp, p), hi in zip(rc.MULTI_SEGS, ends):
            seg = out[lo:hi].reshape(B, cp)
            assert torch.equal(seg[:, :cl], rng.mask_reference(seed, counter, B, cl, p, offset=draws)), (seed, counter, B, cl)
            assert (seg[:, cl:] == 1).all()
            lo, draws = hi, draws + B * cl


@pytest.mark.parametrize("bad", ["int32", "two"])
def test_malformed_counter_raises_value_error(bad):
    ctr = torch.zeros(1, dtype=torch.int32, device="cuda") if bad == "int32" else torch.zeros(2, dtype=torch.int64, device="cuda")
    new = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    ends, ps, clog, cpad = rc.multi_layout()
    calls = [lambda: ops.dropout_mask(1, 0, 0.5, 5, 3, "cuda", dev_counter=ctr),
             lambda: ops.dropout_mask_multi(1, ctr, ends, ps, clog, cpad, new(ends[-1])),
             lambda: ops.normal_fill(1, new(8), ctr),
             lambda: ops.gp_mix(new(4, 8), new(4, 8), None, 1, ctr),
             lambda: ops.gumbel_posterior(new(3, 5), torch.zeros(3, dtype=torch.int64, device="cuda"), None, 1, ctr),
             lambda: ops.gl_init(new(1, 3, 5), ops.GL_SRC_LOG, new(5, 3), new(5, 6), seed=1, dev_counter=ctr),
             lambda: ops.vae_latent_fwd(new(2, 6), new(2, 6), 2, new(4, 6), seed=1, dev_counter=ctr, want_kl=False)]
    for call in calls:
        with pytest.raises(ValueError, match="device counter"):
            call()
