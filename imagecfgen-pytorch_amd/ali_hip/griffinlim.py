"""Griffin-Lim on the device: spectrograms (or the generator's standardised images) back to waveforms -- the
``torchaudio.transforms.GriffinLim`` the reference builds next to every ``Spectrogram``
(``image_scms/audio_mnist.py:62-64,117``: n_fft 255, win 128, default hop 64; ``whalecalls.py:56-59``: 511 / 128 /
hop 24; ``esrf_acoustic.py:40-43``: 1023 / 256 / hop 79) and calls as
``spectrogram_to_audio(img_to_spect(G(...)).exp())``.  The algorithm is ``torchaudio.functional.griffinlim``:

    mag = specgram ** (1/power);  m = momentum / (1 + momentum);  tprev = 0
    angles = rand(re) + i*rand(im)  (uniform [0,1))   or 1 + 0i when rand_init is False
    repeat n_iter:
        inverse = istft(angles * mag, n_fft, hop, win, window, length)
        rebuilt = stft(inverse, n_fft, hop, win, window, center=True, pad_mode="reflect", onesided=True)
        angles  = rebuilt - m * tprev            (skipped when momentum == 0)
        angles  = angles / (|angles| + 1e-16);   tprev = rebuilt
    return istft(angles * mag, ..., length)

torchaudio is not importable in the build container: parity is pinned to ``torch.stft`` / ``torch.istft`` with
torchaudio's parameter mapping (``griffinlim_torch`` below is that statement; tests/test_griffinlim_cpu.py,
tests/test_gpu_griffinlim.py), not to torchaudio itself.  ``length=None`` is ``torch.istft``'s default,
``n_fft + hop*(T-1) - 2*(n_fft//2)`` samples: ``hop*(T-1)`` for even and ``hop*(T-1) + 1`` for odd ``n_fft``.

Matrix form.  The periodic Hann window has ``win`` non-zero samples centred in the ``n_fft`` frame
(``left = (n_fft - win)//2``), so both transforms are small dense matrices over those samples: the forward one is the
front-end's [2F x win] cos | -sin . window matrix, the inverse one [win x 2F] with entries
``c_f cos(2 pi f n / n_fft) w[n] / n_fft`` and ``-c_f sin(.) w[n] / n_fft`` (c_f = 2, 1 for DC and, for even n_fft,
Nyquist, whose imaginary columns are zero).  Frames are overlap-added at ``t*hop + left``, divided by the envelope
``sum_t w^2`` and cut to ``[n_fft//2, n_fft//2 + L)``.  Matrices and envelope are built in fp64 on the host.  Both
products run on the fp32-MFMA GEMM (``ops.conv_fwd``, 1x1); ``ali_gl_init`` / ``ali_gl_ola`` / ``ali_gl_phase``
(csrc/griffinlim.hip) are the steps between them: 4 launches per iteration plus init, final GEMM and final overlap-add.
"""
import math

import torch

from . import ops
from .graphs import GraphCache
from .rng import phase_reference as uniform_reference  # noqa: F401  (the host recipe of ali_gl_init's phases)


def default_length(n_fft, hop, T):
    """samples ``torch.istft(length=None)`` returns for T frames"""
    return n_fft + hop * (T - 1) - 2 * (n_fft // 2)


def dft_matrices(n_fft, win):
    """(forward [2F, win], inverse [win, 2F]) in fp64: rows / columns ``re | im`` over the window's support"""
    F = n_fft // 2 + 1
    left = (n_fft - win) // 2
    n = torch.arange(win, dtype=torch.float64) + left
    f = torch.arange(F, dtype=torch.float64)
    ang = 2.0 * math.pi * f[:, None] * n[None, :] / n_fft                     # [F, win]
    w = torch.hann_window(win, periodic=True, dtype=torch.float64)
    fwd = torch.cat([torch.cos(ang) * w, -torch.sin(ang) * w], dim=0)
    c = torch.full((F,), 2.0, dtype=torch.float64)
    c[0] = 1.0
    ci = c.clone()
    ci[0] = 0.0
    if n_fft % 2 == 0:
        c[-1], ci[-1] = 1.0, 0.0
    inv = torch.cat([(torch.cos(ang) * c[:, None]).T, (-torch.sin(ang) * ci[:, None]).T], dim=1) * (w[:, None] / n_fft)
    return fwd, inv


def envelope(n_fft, win, hop, T):
    """sum_t w^2 over the un-cut overlap-add signal, fp64 [n_fft + hop*(T-1)]"""
    left = (n_fft - win) // 2
    w2 = torch.hann_window(win, periodic=True, dtype=torch.float64) ** 2
    env = torch.zeros(n_fft + hop * (T - 1), dtype=torch.float64)
    for t in range(T):
        env[t * hop + left:t * hop + left + win] += w2
    return env


def reciprocal_envelope(n_fft, win, hop, T, L):
    """the table ``ali_gl_ola`` multiplies by: fp32 of the fp64 reciprocal envelope over the un-cut signal, zero outside
    the kept range [n_fft//2, n_fft//2 + L)"""
    start = n_fft // 2
    env = envelope(n_fft, win, hop, T)
    r = torch.zeros(max(env.numel(), start + L), dtype=torch.float64)
    end = min(start + L, env.numel())
    kept = env[start:end]
    r[start:end] = torch.where(kept > 1e-11, 1.0 / kept.clamp_min(1e-300), torch.zeros_like(kept))
    return r.float()


def reflect_index(n_fft, win, hop, T, L):
    """int64 [T, win]: the un-cut-signal position frame t, tap j of ``torch.stft(center=True, pad_mode="reflect")``
    reads, for a kept signal of L samples starting at n_fft//2"""
    left, start = (n_fft - win) // 2, n_fft // 2
    i = torch.arange(T)[:, None] * hop + left + torch.arange(win)[None, :] - start
    i = torch.where(i < 0, -i, i)
    i = torch.where(i >= L, 2 * (L - 1) - i, i)
    return i + start


def _check_args(n_fft, win, hop, power, momentum, n_iter):
    if not 0.0 <= momentum < 1.0:
        raise ValueError(f"griffinlim: momentum must be in [0, 1), got {momentum}")
    if not power > 0:
        raise ValueError(f"griffinlim: power must be positive, got {power}")
    if n_iter < 0:
        raise ValueError(f"griffinlim: n_iter must be >= 0, got {n_iter}")
    if not 0 < hop <= win <= n_fft:
        raise ValueError(f"griffinlim: need 0 < hop_length <= win_length <= n_fft, got {hop}, {win}, {n_fft}")


def griffinlim_torch(specgram, n_fft, n_iter=32, win_length=None, hop_length=None, power=2.0, momentum=0.99,
                     length=None, rand_init=True, angles0=None):
    """The algorithm of the module docstring with ``torch.stft`` / ``torch.istft`` (any device and float dtype): the CPU
    path of ``WaveformData.spectrogram_to_audio`` and the statement the kernels are tested against."""
    win = win_length or n_fft
    hop = hop_length or win // 2
    _check_args(n_fft, win, hop, power, momentum, n_iter)
    if specgram.shape[-2] != n_fft // 2 + 1:
        raise ValueError(f"griffinlim: expected {n_fft // 2 + 1} frequency bins, got {specgram.shape[-2]}")
    if hop >= win:
        raise ValueError("griffinlim: the Hann window needs hop_length < win_length (torch.istft: window overlap add)")
    shape = specgram.shape
    spec = specgram.reshape((-1,) + tuple(shape[-2:]))
    window = torch.hann_window(win, periodic=True, dtype=spec.dtype, device=spec.device)
    mag = spec.pow(1.0 / power)
    m = momentum / (1 + momentum)
    cdtype = torch.complex128 if spec.dtype == torch.float64 else torch.complex64
    if angles0 is not None:
        angles = angles0.reshape(spec.shape).to(cdtype)
    elif rand_init:
        angles = torch.rand(spec.shape, dtype=cdtype, device=spec.device)
    else:
        angles = torch.full(spec.shape, 1, dtype=cdtype, device=spec.device)
    tprev = torch.tensor(0.0, dtype=spec.dtype, device=spec.device)
    for _ in range(n_iter):
        inverse = torch.istft(angles * mag, n_fft, hop, win, window, length=length)
        rebuilt = torch.stft(inverse, n_fft, hop, win, window, center=True, pad_mode="reflect", normalized=False,
                             onesided=True, return_complex=True)
        angles = rebuilt
        if momentum:
            angles = angles - tprev * m
        angles = angles / (angles.abs() + 1e-16)
        tprev = rebuilt
    wave = torch.istft(angles * mag, n_fft, hop, win, window, length=length)
    return wave.reshape(tuple(shape[:-2]) + wave.shape[-1:])


def _planes(angles0, shape, device):
    """complex [..., F, T] tensor or a (re, im) pair -> two contiguous fp32 [B,F,T] planes on ``device``"""
    re, im = (angles0.real, angles0.imag) if torch.is_tensor(angles0) else angles0
    return tuple(p.reshape(shape).to(device, torch.float32).contiguous() for p in (re, im))


class GriffinLim:
    """``torchaudio.transforms.GriffinLim`` on the HIP kernels (constructor order of the shared arguments as there).

    ``gl(specgram[..., F, T], angles0=None) -> [..., length]`` and ``gl.from_image(img, mean, std, stds_kept)`` straight
    from the generator's standardised output (``img_to_spect``, ``.exp()`` and the root fused into the first launch);
    ``gl.from_log(log_spec)`` takes a log-spectrogram.  Buffers are allocated once per input shape; with ``capture``
    the whole call is recorded once per shape and entry point (``graphs.GraphCache``) and replayed.  Random initial
    phases are keyed by (``seed``, ``gl.counter``): the device counter advances by one per call -- inside the final
    launch, so replays draw fresh phases -- and ``uniform_reference(seed, counter, B*F*T)`` reproduces a call's draws on
    the host.  CPU tensors run ``griffinlim_torch``."""

    def __init__(self, n_fft, n_iter=32, win_length=None, hop_length=None, power=2.0, momentum=0.99, length=None,
                 rand_init=True, device="cuda", seed=0, capture=True):
        self.n_fft, self.n_iter = int(n_fft), int(n_iter)
        self.win = int(win_length or n_fft)
        self.hop = int(hop_length or self.win // 2)
        self.power, self.momentum, self.length, self.rand_init = float(power), float(momentum), length, bool(rand_init)
        self.device, self.seed, self.capture = torch.device(device), int(seed), bool(capture)
        _check_args(self.n_fft, self.win, self.hop, self.power, self.momentum, self.n_iter)
        self.F = self.n_fft // 2 + 1
        if (2 * self.F) % 32 or self.win % 32:
            raise ValueError("2*(n_fft//2 + 1) and win_length must be multiples of 32 (channel stride of the GEMM's "
                             f"fast path), got {2 * self.F} and {self.win}")
        if not ops.gl_check(self.n_fft, self.win, self.hop, 2 + 2 * (self.win // self.hop)):
            raise ValueError(f"griffinlim: hop_length {self.hop} leaves gaps in the overlap-added Hann window of "
                             f"{self.win} samples (torch.istft: window overlap add)")
        self.m = self.momentum / (1 + self.momentum)
        self.fwd64, self.inv64 = dft_matrices(self.n_fft, self.win)
        self._w = None                     # (forward [2F,1,win], inverse [win,1,2F]) on the device
        self.counter = None                # int64 [1] on the device: calls that drew random phases so far
        self._states = {}
        self._graphs = GraphCache()
        self.launches = 0                  # C-ABI launches of the last eager / recorded pass

    # ---- per-shape state
    def _length(self, T):
        L = default_length(self.n_fft, self.hop, T) if self.length is None else int(self.length)
        if L <= self.n_fft // 2:
            raise ValueError(f"griffinlim: {T} frames give {L} samples, reflect padding needs more than {self.n_fft // 2}")
        if 1 + (L + 2 * (self.n_fft // 2) - self.n_fft) // self.hop != T:
            raise ValueError(f"griffinlim: a signal of length {L} does not have the spectrogram's {T} frames")
        if not ops.gl_check(self.n_fft, self.win, self.hop, T, L):
            raise ValueError("griffinlim: window overlap add is zero inside the kept range (torch.istft)")
        return L

    def renv(self, T, L):
        return reciprocal_envelope(self.n_fft, self.win, self.hop, T, L)

    def _upload(self):
        if self._w is None:
            dev = self.device
            self._w = (self.fwd64.float().reshape(2 * self.F, 1, self.win).contiguous().to(dev),
                       self.inv64.float().reshape(self.win, 1, 2 * self.F).contiguous().to(dev))
            self.counter = torch.zeros(1, dtype=torch.int64, device=dev)

    def _state(self, B, T):
        st = self._states.get((B, T))
        if st is None:
            L = self._length(T)
            new = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.device)  # noqa: E731
            st = dict(L=L, renv=self.renv(T, L).to(self.device), mag=new(B * T, self.F), X=new(B * T, 2 * self.F),
                      fr=new(B, T, self.win), frames=new(B, T, self.win), Y=(new(B * T, 2 * self.F), new(B * T, 2 * self.F)),
                      out=new(B, L))
            self._states[(B, T)] = st
        return st

    # ---- the launches
    def _run(self, st, mode, src, a0, stats):
        B, F, T = src.shape
        F2, win = 2 * F, self.win
        n = [0]

        def gemm(x, c_in, w, y, c_out):
            ops.conv_fwd(ops.geom(B, T, 1, c_in, T, 1, c_out, 1, 1, 1, 0), x.view(B, T, 1, c_in), w, y.view(B, T, 1, c_out),
                         ops.epilogue())
            n[0] += 1

        draws = a0 is None and self.rand_init
        mean, std, k = stats if stats is not None else (None, None, 3.0)
        ops.gl_init(src, mode, st["mag"], st["X"], self.power, mean, std, k, a0, self.rand_init, self.seed,
                    self.counter if draws else None)
        for it in range(self.n_iter):
            gemm(st["X"], F2, self._w[1], st["fr"], win)
            ops.gl_ola(st["fr"], st["renv"], self.n_fft, self.hop, st["L"], st["frames"])
            Y = st["Y"][it & 1]
            gemm(st["frames"], win, self._w[0], Y, F2)
            ops.gl_phase(Y, st["Y"][1 - (it & 1)] if (it and self.m) else None, st["mag"], self.m, st["X"])
            n[0] += 2
        gemm(st["X"], F2, self._w[1], st["fr"], win)
        ops.gl_ola(st["fr"], st["renv"], self.n_fft, self.hop, st["L"], st["out"], final=True,
                   advance=self.counter if draws else None)
        self.launches = n[0] + 2
        return st["out"]

    @torch.no_grad()
    def _call(self, mode, src, angles0, stats):
        shape = tuple(src.shape)
        if len(shape) < 2 or shape[-2] != self.F:
            raise ValueError(f"griffinlim: expected [..., {self.F}, T], got {shape}")
        if not src.is_cuda:
            raise ValueError("griffinlim: the kernels need CUDA tensors")
        self._upload()
        src = src.reshape((-1,) + shape[-2:]).float().contiguous()
        B, _, T = src.shape
        st = self._state(B, T)
        a0 = None if angles0 is None else _planes(angles0, src.shape, src.device)
        if stats is not None:
            stats = tuple(s.reshape(-1).to(src.device, torch.float32).contiguous() for s in stats[:2]) + (float(stats[2]),)
            if stats[0].numel() != T or stats[1].numel() != T:
                raise ValueError(f"griffinlim: mean / std must have one entry per frame ({T})")
        if not self.capture:
            out = self._run(st, mode, src, a0, stats)
        else:
            kept = None if stats is None else stats[2]

            def run(s, re, im, mean, std):
                return self._run(st, mode, s, None if re is None else (re, im), None if mean is None else (mean, std, kept))
            # (state: the warm-up is no call -- the same counter value again)
            out = self._graphs(run, (src,) + (a0 or (None, None)) + (stats[:2] if stats is not None else (None, None)),
                               (mode, kept), [self.counter])
        return out.clone().reshape(shape[:-2] + (st["L"],))

    def __call__(self, specgram, angles0=None):
        """specgram [..., F, T] (power spectrogram for power=2) -> waveform [..., length]"""
        if not specgram.is_cuda:
            return griffinlim_torch(specgram, self.n_fft, self.n_iter, self.win, self.hop, self.power, self.momentum,
                                    self.length, self.rand_init, None if angles0 is None else _as_complex(angles0))
        return self._call(ops.GL_SRC_SPEC, specgram, angles0, None)

    def from_log(self, log_spec, angles0=None):
        """``self(log_spec.exp())`` with the exponential fused into the first launch"""
        if not log_spec.is_cuda:
            return self(log_spec.exp(), angles0)
        return self._call(ops.GL_SRC_LOG, log_spec, angles0, None)

    def from_image(self, img, mean, std, stds_kept=3.0, angles0=None):
        """``self(img_to_spect(img, mean, std, stds_kept).exp())`` (audio_mnist.py:365-366: ``img * stds_kept * (std +
        1e-6) + mean``, statistics per last index) for img [..., F, T], e.g. the generator's [B,1,F,T] output"""
        if not img.is_cuda:
            spec = img * stds_kept * (std.reshape(-1) + 1e-6) + mean.reshape(-1)
            return self(spec.exp(), angles0)
        return self._call(ops.GL_SRC_IMAGE, img, angles0, (mean, std, stds_kept))


def _as_complex(angles0):
    return angles0 if torch.is_tensor(angles0) else torch.complex(angles0[0], angles0[1])
