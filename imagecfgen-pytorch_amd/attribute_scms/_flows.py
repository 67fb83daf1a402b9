"""The four transforms the attribute SCMs take from pyro, restated on ``torch.distributions``: pyro is not
needed.  Everything else the family uses -- Normal, Uniform, Categorical, TransformedDistribution, ExpTransform,
SigmoidTransform, AffineTransform -- is torch's own, which is what pyro re-exports.

  BatchNorm(1)                          moving statistics in the sampling direction, batch statistics (unbiased
                                        variance) in the density direction while training
  ConditionalAffineAutoregressive(1,1)  for one variable the MADE masks leave a network of the context alone:
                                        Linear(1, 10) -> ReLU -> Linear(10, 2) = (mean, log_scale)
  ConditionalTransformedDistribution    ``condition(ctx)`` binds the conditional transforms
  Spline(1)                             rational-linear, 8 bins on [-3, 3]^2, identity outside

Each transform with parameters is a ``torch.distributions.Transform`` and an ``nn.Module``: ``t.training = False``,
``t.parameters()``, ``t(x)`` and ``t.inv(y)`` all work.  These definitions are the statement the kernels of
csrc/flow.hip are tested against; they are dtype-generic (``module.double()`` gives the fp64 statement).
They are elementwise (event_dim 0): ``log_prob`` of an [N, 1] value is [N, 1]."""
import torch
import torch.nn.functional as F
from torch import nn
from torch.distributions import SigmoidTransform, Transform, TransformedDistribution, constraints

_F32 = torch.finfo(torch.float32)


class TransformModule(Transform, nn.Module):
    domain = constraints.real
    codomain = constraints.real
    bijective = True
    sign = +1

    def __init__(self):
        super().__init__(cache_size=0)          # Transform's, which goes on to nn.Module's

    __hash__ = nn.Module.__hash__               # (Transform defines __eq__, which would drop it)

    def clear_cache(self):
        pass


class Sigmoid32(SigmoidTransform):
    """SigmoidTransform whose inverse clamps to fp32's [tiny, 1 - eps] in every dtype: the fp64 statement then treats
    the two extreme rows of a data set (p = 0 and p = 1) as the fp32 one and the kernels do."""

    def _inverse(self, y):
        y = y.clamp(min=_F32.tiny, max=1.0 - _F32.eps)
        return y.log() - (-y).log1p()


class BatchNorm(TransformModule):
    def __init__(self, input_dim=1, momentum=0.1, epsilon=1e-5):
        super().__init__()
        self.input_dim, self.momentum, self.epsilon = input_dim, momentum, epsilon
        self.gamma = nn.Parameter(torch.ones(input_dim))
        self.beta = nn.Parameter(torch.zeros(input_dim))
        self.register_buffer("moving_mean", torch.zeros(input_dim))
        self.register_buffer("moving_variance", torch.ones(input_dim))

    @property
    def constrained_gamma(self):
        return F.relu(self.gamma) + 1e-6

    def _call(self, x):
        """the sampling direction: always the moving statistics"""
        return ((x - self.beta) / self.constrained_gamma * torch.sqrt(self.moving_variance + self.epsilon)
                + self.moving_mean)

    def _inverse(self, y):
        """the density direction; training: the batch's mean and unbiased variance, which also move the buffers"""
        if self.training:
            m, v = y.mean(0), y.var(0, unbiased=True)
            with torch.no_grad():
                self.moving_mean.mul_(1 - self.momentum).add_(m * self.momentum)
                self.moving_variance.mul_(1 - self.momentum).add_(v * self.momentum)
        else:
            m, v = self.moving_mean, self.moving_variance
        return (y - m) * torch.rsqrt(v + self.epsilon) * self.constrained_gamma + self.beta

    def log_abs_det_jacobian(self, x, y):
        v = y.var(0, unbiased=True) if self.training else self.moving_variance
        return (-self.constrained_gamma.log() + 0.5 * torch.log(v + self.epsilon)).expand(x.shape)


class _BoundAffine(Transform):
    """y = exp(ls) x + mean with (mean, log_scale) = net(context); ls = clamp(log_scale, -5, 3), straight-through"""
    domain = constraints.real
    codomain = constraints.real
    bijective = True
    sign = +1

    def __init__(self, module, context):
        super().__init__(cache_size=0)
        self.module, self.context = module, context

    def _params(self):
        out = self.module.nn(self.context)
        mean, log_scale = out[..., :1], out[..., 1:]
        lo, hi = self.module.log_scale_min_clip, self.module.log_scale_max_clip
        return mean, log_scale + (log_scale.clamp(lo, hi) - log_scale).detach()

    def _call(self, x):
        mean, ls = self._params()
        return torch.exp(ls) * x + mean

    def _inverse(self, y):
        mean, ls = self._params()
        return (y - mean) * torch.exp(-ls)

    def log_abs_det_jacobian(self, x, y):
        return self._params()[1].expand(x.shape)


class ConditionalAffineAutoregressive(nn.Module):
    def __init__(self, input_dim=1, context_dim=1, hidden_dim=10, log_scale_min_clip=-5.0, log_scale_max_clip=3.0):
        super().__init__()
        if input_dim != 1:
            raise NotImplementedError("only input_dim = 1, where the autoregressive masks leave the context network")
        self.log_scale_min_clip, self.log_scale_max_clip = log_scale_min_clip, log_scale_max_clip
        self.nn = nn.Sequential(nn.Linear(context_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 2))

    def condition(self, context):
        return _BoundAffine(self, context)

    def clear_cache(self):
        pass


def conditional_affine_autoregressive(input_dim, context_dim):
    return ConditionalAffineAutoregressive(input_dim, context_dim)


class ConditionalTransformedDistribution:
    def __init__(self, base_dist, transforms):
        self.base_dist = base_dist
        self.transforms = list(transforms)

    def condition(self, context):
        return TransformedDistribution(self.base_dist, [t.condition(context) if hasattr(t, "condition") else t
                                                        for t in self.transforms])

    def clear_cache(self):
        pass


class Spline(TransformModule):
    """Rational-linear spline (Dolatabadi et al. 2020) of one variable: ``count_bins`` bins on [-bound, bound]^2."""

    def __init__(self, input_dim=1, count_bins=8, bound=3.0):
        super().__init__()
        if input_dim != 1:
            raise NotImplementedError("only input_dim = 1")
        self.count_bins, self.bound = count_bins, bound
        self.unnormalized_widths = nn.Parameter(torch.randn(1, count_bins))
        self.unnormalized_heights = nn.Parameter(torch.randn(1, count_bins))
        self.unnormalized_derivatives = nn.Parameter(torch.randn(1, count_bins - 1))
        self.unnormalized_lambdas = nn.Parameter(torch.randn(1, count_bins))

    def processed(self):
        """knots x [K+1], y [K+1], knot derivatives d [K+1], lambdas [K]"""
        K, B = self.count_bins, self.bound

        def knots(u):
            w = 1e-3 + (1 - 1e-3 * K) * torch.softmax(u[0], dim=-1)
            inner = -B + 2 * B * torch.cumsum(w, dim=-1)[:-1]
            return torch.cat([inner.new_full((1,), -B), inner, inner.new_full((1,), B)])
        ud = self.unnormalized_derivatives[0]
        one = ud.new_ones(1)
        d = torch.cat([one, 1e-3 + F.softplus(ud), one])
        lam = 0.95 * torch.sigmoid(self.unnormalized_lambdas[0]) + 0.025
        return knots(self.unnormalized_widths), knots(self.unnormalized_heights), d, lam

    def _map(self, v, inverse):
        """(the image of v, log |d image / d v|)"""
        xk, yk, d, lam = self.processed()
        B = self.bound
        inside = (v >= -B) & (v <= B)
        vc = v.clamp(-B, B).to(xk.dtype)
        k = (vc.unsqueeze(-1) >= (yk if inverse else xk)[1:-1]).sum(-1)       # the bin: 0 .. K-1
        x0, x1, y0, y1, d0, d1, la = xk[k], xk[k + 1], yk[k], yk[k + 1], d[k], d[k + 1], lam[k]
        w = x1 - x0
        wb = torch.sqrt(d0 / d1)                                                 # (wa = 1)
        wc = (la * d0 + (1 - la) * wb * d1) * w / (y1 - y0)
        yc = ((1 - la) * y0 + la * wb * y1) / ((1 - la) + la * wb)
        if inverse:
            left = vc <= yc
            num = torch.where(left, la * (y0 - vc), (wc - la * wb) * vc + la * wb * y1 - wc * yc)
            den = torch.where(left, (wc - 1) * vc + y0 - wc * yc, (wc - wb) * vc + wb * y1 - wc * yc)
            out = num / den * w + x0
            deriv = torch.where(left, wc * la * (yc - y0), wb * wc * (1 - la) * (y1 - yc)) * w / den ** 2
        else:
            th = (vc - x0) / w
            left = th <= la
            num = torch.where(left, y0 * (la - th) + wc * yc * th, wc * yc * (1 - th) + wb * y1 * (th - la))
            den = torch.where(left, (la - th) + wc * th, wc * (1 - th) + wb * (th - la))
            out = num / den
            deriv = torch.where(left, wc * la * (yc - y0), wb * wc * (1 - la) * (y1 - yc)) / w / den ** 2
        return torch.where(inside, out, v.to(out.dtype)), torch.where(inside, deriv.log(), torch.zeros_like(out))

    def _call(self, x):
        return self._map(x, False)[0]

    def _inverse(self, y):
        return self._map(y, True)[0]

    def log_abs_det_jacobian(self, x, y):
        return self._map(x, False)[1]
