"""GPU parity of Griffin-Lim (csrc/griffinlim.hip, ``ali_hip.griffinlim.GriffinLim``).

Reference: the fp64 restatement of torchaudio's loop with ``torch.stft`` / ``torch.istft`` (test_griffinlim_cpu.py).
Yardstick (as in test_gpu_ssim.py): the fp32 evaluation of the MATRIX form on the CPU -- an equally valid fp32
summation order of the same direct DFT -- against that reference on the same inputs.  The device may deviate from the
reference by at most 4x that, plus an absolute floor of 1e-7 * max|reference| per element.  The fp32 FFT is no
yardstick: a direct 256..1024-term sum is several times less exact than the butterflies.

Shapes are (n_fft, win, hop, B, T); the spectrogram of T frames comes from a signal of ``hop*(T-1) + n_fft % 2``
samples, ``torch.istft``'s default length for T frames (see test_griffinlim_cpu.py).
"""
import functools

import pytest
import torch
import torch.nn.functional as Fn

from test_griffinlim_cpu import SHAPES, inputs, matrix_form, reference, restate

pytestmark = pytest.mark.gpu


def _gl(shape, **kw):
    from ali_hip.griffinlim import GriffinLim
    return GriffinLim(shape[0], win_length=shape[1], hop_length=shape[2], **kw)


@functools.lru_cache(maxsize=None)
def yard(shape, n_iter):
    """(waveform, last rebuilt or None) of the fp32 matrix form on the CPU: computed once"""
    spec, a0 = inputs(shape)
    keep = []
    w = matrix_form(spec.float(), *shape[:3], n_iter, a0.to(torch.complex64), torch.float32, keep=keep)
    return w, (keep[0] if keep else None)


def within_yardstick(got, ref, yardstick, what):
    """||got - ref||_2 <= 4 ||yardstick - ref||_2 + 1e-7 max|ref| sqrt(n); returns the relative allowance"""
    if torch.is_complex(ref):
        got, ref, yardstick = (torch.view_as_real(t.cpu().to(torch.complex128).contiguous()) for t in (got, ref, yardstick))
    got, ref, yardstick = got.double().cpu(), ref.double(), yardstick.double()
    err, dev = (got - ref).norm().item(), (yardstick - ref).norm().item()
    floor = 1e-7 * ref.abs().max().item() * ref.numel() ** 0.5
    n = ref.norm().item()
    print(f"{what}: rel-L2 {err / n:.3e} (fp32 matrix form on the CPU {dev / n:.3e}, floor {floor / n:.1e})")
    assert torch.isfinite(got).all()
    assert err <= 4 * dev + floor, (what, err / n, dev / n)
    return (4 * dev + floor) / n


def _spectrum(Y, B, T, F):
    """[B*T, 2F] re | im -> complex [B,F,T]"""
    Y = Y.double().cpu().reshape(B, T, 2 * F)
    return torch.complex(Y[..., :F], Y[..., F:]).transpose(1, 2)


# ---- 1. per kernel -----------------------------------------------------------------------------------------------------
def _exact_ola(fr, n_fft, hop):
    B, T, win = fr.shape
    y = torch.zeros(B, n_fft + hop * (T - 1), dtype=torch.float64)
    for t in range(T):
        y[:, t * hop + (n_fft - win) // 2:][:, :win] += fr[:, t].double()
    return y


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fpb", [0, 3])
def test_ola_is_exact_on_integers(shape, fpb):
    """Small-integer frames: every sum is exact, so the waveform is (exact sum) * renv bit for bit and the re-framed
    output an exact copy of F.pad(reflect) + unfold of it -- offsets, reflect map, edges, block seams (``fpb`` = frames
    per block: 3 puts seams everywhere; 0, the launch's own choice, gives 4 blocks at T = 128), ``length`` trim."""
    from ali_hip import griffinlim as gl, ops
    n_fft, win, hop, B, T = shape
    G = _gl(shape)
    left, start = (n_fft - win) // 2, n_fft // 2
    g = torch.Generator().manual_seed(T)
    fr = torch.randint(-8, 9, (B, T, win), generator=g).float()
    y = _exact_ola(fr, n_fft, hop)
    L0 = gl.default_length(n_fft, hop, T)
    for L in (L0, L0 - 3, L0 + min(5, hop - 1)):
        renv = G.renv(T, L)
        wave = (y.float() * renv[:y.shape[1]])[:, start:start + L]             # fp32 product of the exact sum
        out = torch.full((B, L), float("nan"), device="cuda")
        ops.gl_ola(fr.cuda(), renv.cuda(), n_fft, hop, L, out, final=True, frames_per_block=fpb)
        assert torch.equal(out.cpu(), wave), (L, "waveform")
        if L < L0:
            continue                                                            # (a shorter signal has T-1 frames)
        frames = Fn.pad(wave[:, None], (start, start), mode="reflect")[:, 0][:, left:].unfold(1, win, hop)[:, :T]
        out = torch.full((B, T, win), float("nan"), device="cuda")
        ops.gl_ola(fr.cuda(), renv.cuda(), n_fft, hop, L, out, frames_per_block=fpb)
        assert torch.equal(out.cpu(), frames.contiguous()), (L, "frames")


def test_ola_zero_pads_behind_the_signal_and_advances_the_counter():
    """``length`` past the signal's end (legal for torch.istft only where the window covers the whole tail: n_fft ==
    win): zeros there; the final launch adds one to the device counter"""
    from ali_hip import griffinlim as gl, ops
    n_fft, win, hop, B, T = 128, 128, 32, 2, 7
    fr = torch.randint(-8, 9, (B, T, win), generator=torch.Generator().manual_seed(1)).float()
    y = _exact_ola(fr, n_fft, hop)
    Lp = y.shape[1] - 64 + 7
    assert ops.gl_check(n_fft, win, hop, T, Lp)
    renv = gl.reciprocal_envelope(n_fft, win, hop, T, Lp)
    wave = Fn.pad((y.float() * renv[:y.shape[1]])[:, 64:], (0, 7))
    for fpb in (0, 2):
        ctr = torch.full((1,), 41, dtype=torch.int64, device="cuda")
        out = torch.full((B, Lp), float("nan"), device="cuda")
        ops.gl_ola(fr.cuda(), renv.cuda(), n_fft, hop, Lp, out, final=True, frames_per_block=fpb, advance=ctr)
        assert torch.equal(out.cpu(), wave) and ctr.item() == 42


def test_ola_against_torch_istft():
    """real inverse frames: waveform vs torch.istft (fp64) to fp32 rounding of a sum of <= 6 terms"""
    from ali_hip import griffinlim as gl, ops
    for shape in SHAPES[:3]:
        n_fft, win, hop, B, T = shape
        spec, a0 = inputs(shape)
        S = a0 * spec.sqrt()
        ref = torch.istft(S, n_fft, hop, win, torch.hann_window(win, dtype=torch.float64))
        fr = (torch.cat([S.real, S.imag], 1).transpose(1, 2) @ gl.dft_matrices(n_fft, win)[1].T).float()
        L = ref.shape[1]
        out = torch.empty(B, L, device="cuda")
        ops.gl_ola(fr.cuda().contiguous(), _gl(shape).renv(T, L).cuda(), n_fft, hop, L, out, final=True)
        # 8 roundings (frames, <= 6 additions, envelope, product) of values <= max|frame| / min envelope
        tol = 8 * 2.0 ** -24 * fr.abs().max().item() * _gl(shape).renv(T, L).max().item()
        assert (out.double().cpu() - ref).abs().max().item() <= tol


def test_phase_kernel():
    """|a| >= 0.1 everywhere except a block of exact zeros.  a = Y - m*tprev carries <= 3 roundings of values <= 2
    (4e-7 absolute), 4e-6 relative to |a| >= 0.1; the quotient and two products add a few 2^-24: 2e-5 * mag bounds it."""
    from ali_hip import ops
    rows, F, m = 37, 144, 0.99 / 1.99
    g = torch.Generator().manual_seed(3)
    tprev = torch.rand(rows, 2 * F, generator=g) * 2 - 1
    ang, mod = torch.rand(rows, F, generator=g) * 6.2832, torch.rand(rows, F, generator=g) * 0.9 + 0.15
    a = torch.cat([mod * ang.cos(), mod * ang.sin()], dim=1)
    Y = a + m * tprev
    Y[5:9], tprev[5:9] = 0.0, 0.0
    mag = torch.rand(rows, F, generator=g) * 3
    for tp, mm in ((tprev, m), (None, m), (tprev, 0.0)):
        X = torch.full((rows, 2 * F), float("nan"), device="cuda")
        ops.gl_phase(Y.cuda(), None if tp is None else tp.cuda(), mag.cuda(), mm, X)
        ad = Y.double() - (mm * tp.double() if (tp is not None and mm) else 0)
        ac = torch.complex(ad[:, :F], ad[:, F:])
        assert tp is None or mm == 0 or ac[torch.arange(rows) >= 9].abs().min() >= 0.1
        ref = ac / (ac.abs() + 1e-16) * mag.double()
        got = _spectrum(X, 1, rows, F)[0].transpose(0, 1)
        assert torch.isfinite(X).all()
        assert ((got - ref).abs() <= 2e-5 * mag.double() + 1e-30).all()
        if tp is not None:
            assert (X[5:9] == 0).all()


def test_init_kernel_modes_transposition_and_draws():
    """F, T no multiples of the 32x32 tile, three batches.  mag: <= 3 roundings in front of an exponential of argument
    <= 8 in size (3 * 16 * 2^-24 = 3e-6 relative) plus the function's own few ulps: 5e-6 relative."""
    from ali_hip import ops
    from ali_hip.griffinlim import uniform_reference
    B, F, T = 3, 45, 19
    g = torch.Generator().manual_seed(4)
    img = torch.rand(B, F, T, generator=g) * 2 - 1
    mean, std = torch.randn(T, generator=g), torch.rand(T, generator=g) + 0.5
    a0 = (torch.rand(B, F, T, generator=g), torch.rand(B, F, T, generator=g))
    new = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    cases = [(ops.GL_SRC_IMAGE, img, ((img.double() * 3 * (std.double() + 1e-6) + mean.double()) / 2).exp(), 2.0),
             (ops.GL_SRC_LOG, img * 8, (img.double() * 8 / 2).exp(), 2.0),
             (ops.GL_SRC_SPEC, (img * 4).exp(), (img * 4).exp().double().sqrt(), 2.0),
             (ops.GL_SRC_SPEC, (img * 4).exp(), (img * 4).exp().double(), 1.0),
             (ops.GL_SRC_SPEC, (img * 4).exp(), (img * 4).exp().double().pow(1 / 3), 3.0)]
    for mode, src, ref, power in cases:
        mag, X = new(B * T, F), new(B * T, 2 * F)
        ops.gl_init(src.cuda(), mode, mag, X, power, mean.cuda(), std.cuda(), 3.0, tuple(p.cuda() for p in a0))
        ref = ref.transpose(1, 2).reshape(B * T, F)
        assert ((mag.double().cpu() - ref).abs() <= 5e-6 * ref).all(), mode
        for part, plane in zip((X[:, :F], X[:, F:]), a0):                      # X = (re | im) * mag, one fp32 product
            assert torch.equal(part.cpu(), plane.transpose(1, 2).reshape(B * T, F) * mag.cpu())
    ones = torch.ones(B, F, T, device="cuda")
    mag, X = new(B * T, F), new(B * T, 2 * F)
    ops.gl_init(ones, ops.GL_SRC_SPEC, mag, X, rand_init=False)                # no draw: 1 + 0i
    assert (X[:, :F] == 1).all() and (X[:, F:] == 0).all() and (mag == 1).all()
    ctr = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    ops.gl_init(ones, ops.GL_SRC_SPEC, mag, X, seed=77, dev_counter=ctr)       # mag = 1: X holds the draws themselves
    u = uniform_reference(77, 9, B * F * T).reshape(2, B, F, T).transpose(2, 3).reshape(2, B * T, F)
    assert torch.equal(X[:, :F].cpu(), u[0]) and torch.equal(X[:, F:].cpu(), u[1])
    X2 = new(B * T, 2 * F)                                                      # split at an odd offset = one launch
    assert (F * T) % 2 == 1
    ops.gl_init(ones[:1], ops.GL_SRC_SPEC, mag[:T], X2[:T], seed=77, dev_counter=ctr)
    ops.gl_init(ones[1:], ops.GL_SRC_SPEC, mag[T:], X2[T:], seed=77, dev_counter=ctr, offset=F * T)
    assert torch.equal(X2, X)
    ops.gl_init(ones, ops.GL_SRC_SPEC, mag, X2, seed=78, dev_counter=ctr)
    assert not torch.equal(X2, X)


# ---- 2. one iteration and none -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_iter", [0, 1])
def test_first_iteration(shape, n_iter):
    n_fft, win, hop, B, T = shape
    spec, a0 = inputs(shape)
    G = _gl(shape, n_iter=n_iter, capture=False)
    wave = G(spec.float().cuda(), a0.to(torch.complex64).cuda())
    ref, rebuilt = reference(shape, n_iter)
    yw, yr = yard(shape, n_iter)
    assert wave.shape == ref.shape and G.launches == 4 * n_iter + 3
    within_yardstick(wave, ref, yw, f"{shape} n_iter={n_iter} waveform")
    if n_iter:
        within_yardstick(_spectrum(G._states[(B, T)]["Y"][0], B, T, G.F), rebuilt, yr, f"{shape} rebuilt")


# ---- 3. the class defaults ---------------------------------------------------------------------------------------------
def _convergence(wave, spec, shape):
    """|| |STFT(wave)| - mag || / ||mag|| in fp64 on the host"""
    n_fft, win, hop = shape[:3]
    S = torch.stft(wave.double().cpu(), n_fft, hop, win, torch.hann_window(win, dtype=torch.float64), center=True,
                   pad_mode="reflect", onesided=True, return_complex=True)
    return ((S.abs() - spec.sqrt()).norm() / spec.sqrt().norm()).item(), S


@pytest.mark.parametrize("shape", SHAPES)
def test_32_iterations_class_defaults(shape):
    """The waveform under the yardstick; the spectral convergence within the yardstick's deviation carried into the
    spectral domain (| ||a| - mag| - ||b| - mag| | <= |a - b|, so 4 ||STFT(w_yard - w_ref)|| / ||mag|| + the floor bounds
    what 4x the yardstick's own waveform deviation can move it), and lower than without iterations."""
    spec, a0 = inputs(shape)
    G = _gl(shape)                                                              # 32 iterations, momentum 0.99, captured
    wave = G(spec.float().cuda(), a0.to(torch.complex64).cuda())
    ref, _ = reference(shape, 32)
    yw, _ = yard(shape, 32)
    assert G.launches == 4 * 32 + 3
    within_yardstick(wave, ref, yw, f"{shape} 32 iterations waveform")
    sc, _ = _convergence(wave, spec, shape)
    sc_ref, S_ref = _convergence(ref, spec, shape)
    _, S_yard = _convergence(yw, spec, shape)
    allow = 4 * ((S_yard - S_ref).norm() / spec.sqrt().norm()).item() + 1e-7
    sc0, _ = _convergence(reference(shape, 0)[0], spec, shape)
    print(f"{shape}: spectral convergence {sc:.6f} (reference {sc_ref:.6f}, allowance {allow:.2e}; n_iter=0: {sc0:.3f})")
    assert abs(sc - sc_ref) <= allow and sc < sc0


def test_zero_spectrogram_and_momentum_zero():
    shape = SHAPES[1]
    n_fft, win, hop, B, T = shape
    spec, a0 = inputs(shape)
    G = _gl(shape, n_iter=3)
    w = G(torch.zeros(B, n_fft // 2 + 1, T, device="cuda"))
    assert w.shape == (B, hop * (T - 1) + 1) and (w == 0).all()
    G0 = _gl(shape, n_iter=3, momentum=0.0)
    a32 = a0.to(torch.complex64)
    ref = restate(spec, n_fft, win, hop, n_iter=3, angles0=a0, momentum=0.0)
    yw = matrix_form(spec.float(), n_fft, win, hop, 3, a32, torch.float32, momentum=0.0)
    within_yardstick(G0(spec.float().cuda(), a32.cuda()), ref, yw, f"{shape} momentum 0")


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_draws_fresh_phases():
    from ali_hip.griffinlim import uniform_reference
    shape = SHAPES[0]
    n_fft, win, hop, B, T = shape
    spec, a0 = inputs(shape)
    s, a = spec.float().cuda(), a0.to(torch.complex64).cuda()
    Gg, Ge = _gl(shape, n_iter=4, seed=5), _gl(shape, n_iter=4, seed=5, capture=False)
    eager = Ge(s, a)
    assert torch.equal(Gg(s, a), eager) and torch.equal(Gg(s, a), eager)        # first call (capture) and a replay
    assert Gg.counter.item() == 0                                               # given phases: nothing drawn
    w = [Gg(s) for _ in range(3)]                                               # capture at counter 0, then replays
    assert Gg.counter.item() == 3
    assert not torch.equal(w[0], w[1]) and not torch.equal(w[1], w[2])
    Gg.counter.fill_(1)
    assert torch.equal(Gg(s), w[1])                                             # same counter value: same bits
    for c in range(3):
        u = uniform_reference(5, c, B * Gg.F * T).reshape(2, B, Gg.F, T)
        assert torch.equal(Ge(s, (u[0], u[1])), w[c]), c
    Ge.counter.fill_(2)
    assert torch.equal(Ge(s), w[2]) and Ge.counter.item() == 3                  # eager draws advance it as well


# ---- 5. from the generator's image -------------------------------------------------------------------------------------
def test_from_image_and_data_source():
    from image_scms import _spect
    shape = SHAPES[0]
    n_fft, win, hop, B, T = shape
    spec, a0 = inputs(shape)
    log_spec = (spec + 1e-6).log()
    mean, std = log_spec.mean(dim=(0, 1)), log_spec.std(dim=(0, 1))
    img = (torch.clip((log_spec - mean) / (std + 1e-6), -3, 3) / 3).float()     # what G's tanh output looks like
    spec_img = _spect.img_to_spect(img.double(), mean, std).exp()
    a32 = a0.to(torch.complex64)
    ref = restate(spec_img, n_fft, win, hop, n_iter=8, angles0=a0)
    yw = matrix_form(_spect.img_to_spect(img, mean.float(), std.float()).exp(), n_fft, win, hop, 8, a32, torch.float32)
    G = _gl(shape, n_iter=8)
    m, sd = mean.float().cuda(), std.float().cuda()
    within_yardstick(G.from_image(img.cuda().reshape(B, 1, -1, T), m.reshape(1, 1, -1), sd.reshape(1, 1, -1),
                                  angles0=a32.cuda()).reshape(B, -1), ref, yw, "from_image")
    within_yardstick(G(_spect.img_to_spect(img.cuda(), m, sd).exp(), a32.cuda()), ref, yw, "exp(img_to_spect)")
    data = _spect.WaveformData(torch.zeros(B, 16), {}, n_fft=n_fft, win_length=win, device="cuda")
    wav = data.inv_transforms["audio"](log_spec.float().numpy())
    assert wav.is_cuda and wav.shape == (B, hop * (T - 1) + 1) and torch.isfinite(wav).all()
    ref_l = restate(log_spec.exp(), n_fft, win, hop, angles0=a0)
    yl = matrix_form(log_spec.float().exp(), n_fft, win, hop, 32, a32, torch.float32)
    within_yardstick(data.image_to_audio(log_spec.float().cuda(), a32.cuda()), ref_l, yl, "image_to_audio")
    silent = data.spectrogram_to_audio(torch.zeros(B, n_fft // 2 + 1, T, device="cuda"))
    assert (silent == 0).all()
