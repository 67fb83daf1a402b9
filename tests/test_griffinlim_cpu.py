"""Griffin-Lim without a GPU: the host side of ``ali_hip.griffinlim`` (DFT matrices, window envelope, reflect map, RNG
recipe, argument checks) and the CPU path of ``WaveformData.spectrogram_to_audio`` against this file's own restatement
of ``torchaudio.functional.griffinlim`` with ``torch.stft`` / ``torch.istft``.

Shapes are (n_fft, win, hop, B, T).  A spectrogram with T frames comes from a signal of ``torch.istft``'s default
length for T frames, ``hop*(T-1) + n_fft % 2``: with the reference's odd n_fft a signal of ``hop*(T-1)`` samples has
T-1 frames, and ``torch.istft(length=None)`` returns ``hop*(T-1) + 1`` samples.
"""
import functools
import math

import numpy as np
import pytest
import torch

SHAPES = [(255, 128, 64, 2, 8), (511, 128, 24, 1, 19), (1023, 256, 79, 3, 11), (255, 128, 64, 2, 128)]


def restate(spec, n_fft, win, hop, n_iter=32, angles0=None, power=2.0, momentum=0.99, length=None, keep=None):
    """torchaudio.functional.griffinlim, statement by statement, on [B,F,T]; ``angles0`` replaces the random phases.
    ``keep`` (a list) receives the last ``rebuilt``."""
    window = torch.hann_window(win, periodic=True, dtype=spec.dtype)
    momentum = momentum / (1 + momentum)
    specgram = spec.pow(1 / power)
    angles = angles0.clone()
    tprev = torch.tensor(0.0, dtype=spec.dtype)
    for _ in range(n_iter):
        inverse = torch.istft(angles * specgram, n_fft=n_fft, hop_length=hop, win_length=win, window=window, length=length)
        rebuilt = torch.stft(inverse, n_fft=n_fft, hop_length=hop, win_length=win, window=window, center=True,
                             pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
        angles = rebuilt
        if momentum:
            angles = angles - tprev.mul_(momentum)
        angles = angles.div(angles.abs().add(1e-16))
        tprev = rebuilt
        if keep is not None:
            keep[:] = [rebuilt]
    return torch.istft(angles * specgram, n_fft=n_fft, hop_length=hop, win_length=win, window=window, length=length)


def matrix_form(spec, n_fft, win, hop, n_iter, angles0, dtype, power=2.0, momentum=0.99, keep=None):
    """The same loop with the host matrices, envelope and reflect map of ``ali_hip.griffinlim`` applied by ``matmul`` and
    indexing in ``dtype``, in the order the kernels use (frames added in ascending t, times the reciprocal envelope)."""
    from ali_hip import griffinlim as gl
    B, F, T = spec.shape
    left, start = (n_fft - win) // 2, n_fft // 2
    L = gl.default_length(n_fft, hop, T)
    fwd, inv = (m.to(dtype) for m in gl.dft_matrices(n_fft, win))
    env = gl.envelope(n_fft, win, hop, T)
    renv = torch.zeros_like(env)
    renv[start:start + L] = 1.0 / env[start:start + L]
    renv = renv.to(dtype)
    idx = gl.reflect_index(n_fft, win, hop, T, L)
    mag = spec.to(dtype).pow(1 / power).transpose(1, 2)                         # [B,T,F]
    a0 = angles0.transpose(1, 2)
    X = torch.cat([a0.real.to(dtype) * mag, a0.imag.to(dtype) * mag], dim=2)    # [B,T,2F]
    m = momentum / (1 + momentum)

    def ola(fr):
        y = torch.zeros(B, env.numel(), dtype=dtype)
        for t in range(T):
            y[:, t * hop + left:t * hop + left + win] += fr[:, t]
        return y * renv

    tprev = None
    for _ in range(n_iter):
        y = ola(X @ inv.T)
        Y = y[:, idx] @ fwd.T                                                   # [B,T,2F]
        a = Y if (tprev is None or not m) else Y - m * tprev
        s = 1.0 / (torch.hypot(a[..., :F], a[..., F:]) + 1e-16)
        X = torch.cat([a[..., :F] * s * mag, a[..., F:] * s * mag], dim=2)
        tprev = Y
        if keep is not None:
            keep[:] = [torch.complex(Y[..., :F], Y[..., F:]).transpose(1, 2)]
    return ola(X @ inv.T)[:, start:start + L]


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(power spectrogram fp64 [B,F,T], fixed initial phases complex128 [B,F,T]) of a shape"""
    from ali_hip import griffinlim as gl
    n_fft, win, hop, B, T = shape
    g = torch.Generator().manual_seed(1234 + T)
    n = gl.default_length(n_fft, hop, T)
    x = torch.randn(B, n, dtype=torch.float64, generator=g) * torch.linspace(0.1, 1.0, n, dtype=torch.float64)
    S = torch.stft(x, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), center=True, pad_mode="reflect",
                   onesided=True, return_complex=True)
    assert S.shape == (B, n_fft // 2 + 1, T)
    a0 = torch.complex(torch.rand(S.shape, dtype=torch.float64, generator=g), torch.rand(S.shape, dtype=torch.float64, generator=g))
    return S.abs().pow(2.0), a0


@functools.lru_cache(maxsize=None)
def reference(shape, n_iter):
    """(waveform, last rebuilt or None) of the fp64 restatement: computed once, shared, never modified"""
    spec, a0 = inputs(shape)
    keep = []
    w = restate(spec, *shape[:3], n_iter=n_iter, angles0=a0, keep=keep)
    return w, (keep[0] if keep else None)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("shape", SHAPES)
def test_matrix_form_reproduces_stft_istft(shape):
    """fp64, 32 iterations: the matrices, the envelope and the reflect map are the transform (rel-L2 <= 1e-9; a wrong
    tap, offset or c_f gives O(1))."""
    spec, a0 = inputs(shape)
    ref, _ = reference(shape, 32)
    got = matrix_form(spec, *shape[:3], 32, a0, torch.float64)
    assert got.shape == ref.shape
    err = rel_l2(got, ref)
    print(f"{shape}: matrix form vs torch.stft/istft, fp64, 32 iterations: rel-L2 {err:.3e}")
    assert err <= 1e-9


def test_even_n_fft_nyquist_column():
    """even n_fft: Nyquist bin has c_f = 1 and a zero imaginary column (no reference setting is even)"""
    from ali_hip import griffinlim as gl
    n_fft, win, hop, T = 256, 128, 32, 9
    g = torch.Generator().manual_seed(5)
    S = torch.randn(2, 129, T, dtype=torch.complex128, generator=g)
    ref = torch.istft(S, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64))
    _, inv = gl.dft_matrices(n_fft, win)
    fr = torch.cat([S.real, S.imag], 1).transpose(1, 2) @ inv.T
    env = gl.envelope(n_fft, win, hop, T)
    y = torch.zeros(2, env.numel(), dtype=torch.float64)
    for t in range(T):
        y[:, t * hop + 64:t * hop + 64 + win] += fr[:, t]
    got = (y / env.clamp_min(1e-300))[:, 128:128 + ref.shape[1]]
    assert ref.shape[1] == gl.default_length(n_fft, hop, T) == hop * (T - 1)
    assert rel_l2(got, ref) <= 1e-12


def _source(shape, device="cpu", **kw):
    from image_scms import _spect
    n_fft, win, hop, B, T = shape
    return _spect.WaveformData(torch.zeros(B, 16), {}, n_fft=n_fft, win_length=win, hop_length=hop, device=device, **kw)


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_cpu_path_equals_restatement_fp32(shape):
    spec, a0 = inputs(shape)
    spec32, a32 = spec.float(), a0.to(torch.complex64)
    got = _source(shape).spectrogram_to_audio(spec32, angles0=a32)
    ref = restate(spec32, *shape[:3], angles0=a32)
    assert got.dtype == torch.float32 and torch.equal(got, ref)


def test_image_entries_apply_exp_and_img_to_spect():
    from image_scms import _spect, audio_mnist
    shape = SHAPES[0]
    spec, a0 = inputs(shape)
    log_spec, a32 = (spec.float() + 1e-6).log(), a0.to(torch.complex64)
    data = _source(shape, griffin_lim=audio_mnist.GRIFFIN_LIM)
    assert data.griffin_lim == dict(n_fft=255, win_length=128)
    ref = restate(log_spec.exp(), *shape[:3], angles0=a32)
    assert torch.equal(data.image_to_audio(log_spec, angles0=a32), ref)
    torch.manual_seed(11)                                   # inv_transforms draws its phases like the reference: torch.rand
    via_numpy = data.inv_transforms["audio"](log_spec.numpy())
    torch.manual_seed(11)
    a_rand = torch.rand(log_spec.shape, dtype=torch.complex64)
    assert via_numpy.shape == (shape[3], shape[2] * (shape[4] - 1) + 1)
    assert torch.equal(via_numpy, restate(log_spec.exp(), *shape[:3], angles0=a_rand))
    torch.manual_seed(11)
    assert torch.equal(data.inv_transforms["audio"](log_spec), via_numpy)
    # img_to_spect: the reference's statement (audio_mnist.py:365-366)
    g = torch.Generator().manual_seed(2)
    img = torch.rand(2, 1, 128, 8, generator=g) * 2 - 1
    mean, std = torch.randn(1, 1, 8, generator=g), torch.rand(1, 1, 8, generator=g)
    assert torch.equal(_spect.img_to_spect(img, mean, std), img * 3 * (std + 1e-6) + mean)
    assert torch.equal(_spect.img_to_spect(img, mean, std, 2), img * 2 * (std + 1e-6) + mean)


def test_family_settings_are_the_references():
    from image_scms import audio_mnist, esrf_acoustic, whalecalls
    assert audio_mnist.GRIFFIN_LIM == dict(n_fft=255, win_length=128)
    assert whalecalls.GRIFFIN_LIM == dict(n_fft=511, win_length=128, hop_length=24)
    assert esrf_acoustic.GRIFFIN_LIM == dict(n_fft=1023, win_length=256, hop_length=79)
    for mod, hop in ((audio_mnist, 64), (whalecalls, 24), (esrf_acoustic, 79)):
        from ali_hip.griffinlim import GriffinLim
        gl = GriffinLim(**mod.GRIFFIN_LIM)
        assert (gl.hop, gl.n_iter, gl.power, gl.momentum, gl.rand_init, gl.length) == (hop, 32, 2.0, 0.99, True, None)
        assert (2 * gl.F) % 32 == 0


def test_argument_checks():
    from ali_hip.griffinlim import GriffinLim, griffinlim_torch
    for kw in (dict(momentum=1.0), dict(momentum=-0.1), dict(power=0.0), dict(power=-1.0), dict(n_iter=-1),
               dict(hop_length=200),            # hop > win
               dict(hop_length=128),            # hop == win: the Hann window's zero leaves gaps (torch.istft raises)
               dict(win_length=100)):           # not a multiple of 32
        with pytest.raises(ValueError):
            GriffinLim(255, **{**dict(win_length=128), **kw})
    with pytest.raises(ValueError):
        GriffinLim(250, win_length=128)         # 2F = 252
    spec, a0 = inputs(SHAPES[0])
    with pytest.raises(ValueError):
        griffinlim_torch(spec[:, :100], 255, win_length=128, angles0=a0[:, :100])       # wrong F
    with pytest.raises(ValueError):
        griffinlim_torch(spec, 255, win_length=128, hop_length=200, angles0=a0)
    with pytest.raises(ValueError):
        griffinlim_torch(spec, 255, win_length=128, momentum=1.5, angles0=a0)
    gl = GriffinLim(255, win_length=128)
    with pytest.raises(ValueError):
        gl._length(1)                           # one frame: 1 sample, reflect padding impossible
    gl.length = 100
    with pytest.raises(ValueError):
        gl._length(8)                           # 100 samples do not have 8 frames
    # n_iter = 0 and momentum = 0 are legal
    w0 = griffinlim_torch(spec, 255, n_iter=0, win_length=128, angles0=a0)
    assert torch.equal(w0, torch.istft(a0 * spec.sqrt(), 255, 64, 128, torch.hann_window(128, dtype=torch.float64)))
    assert torch.equal(griffinlim_torch(spec, 255, n_iter=2, win_length=128, momentum=0.0, angles0=a0),
                       restate(spec, 255, 128, 64, n_iter=2, angles0=a0, momentum=0.0))


@pytest.mark.parametrize("cfg", [(255, 128, 64, 8, 0), (511, 128, 24, 19, 0), (1023, 256, 79, 11, 0), (255, 128, 128, 6, 0),
                                 (256, 256, 256, 4, 0), (256, 128, 96, 6, 0), (255, 128, 64, 8, 300), (128, 128, 127, 5, 0)])
def test_envelope_check_agrees_with_torch_istft(cfg):
    """ali_gl_check (host function of the library) says what torch.istft's window-overlap check says"""
    from ali_hip import ops
    n_fft, win, hop, T, length = cfg
    S = torch.ones(1, n_fft // 2 + 1, T, dtype=torch.complex128)
    try:
        torch.istft(S, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), length=length or None)
        ok = True
    except RuntimeError:
        ok = False
    assert ops.gl_check(n_fft, win, hop, T, length) == ok
    with pytest.raises(ValueError):
        ops.gl_check(n_fft, win, win + 1, T)


def test_uniform_reference_recipe():
    from ali_hip.griffinlim import uniform_reference
    u = uniform_reference(7, 3, 5000)
    assert u.shape == (2, 5000) and u.dtype == torch.float32
    assert u.min() >= 0 and u.max() < 1
    assert torch.equal(u * 16777216, (u * 16777216).round())                   # 24-bit fields: exact in fp32
    assert abs(u.mean().item() - 0.5) < 0.02 and abs(u.var().item() - 1 / 12) < 0.01
    pieces = torch.cat([uniform_reference(7, 3, 1237), uniform_reference(7, 3, 5000 - 1237, offset=1237)], dim=1)
    assert torch.equal(pieces, u)
    assert not torch.equal(uniform_reference(8, 3, 5000), u)
    assert not torch.equal(uniform_reference(7, 4, 5000), u)
    assert not torch.equal(u[0], u[1])
