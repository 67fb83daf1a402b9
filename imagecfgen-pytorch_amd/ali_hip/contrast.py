"""The contrastive family: the two baseline explainers ``morphomnist_cf_metrics.py`` / ``mnist_oracle_scores.py`` take
from the omnixai package -- ``ContrastiveExplainer(...).explain(...).explanations[0]['pn']`` (pertinent negatives of
the contrastive explanation method, Dhurandhar et al. 2018) and ``CounterfactualExplainer(...)...['cf']`` (Wachter et
al. 2017) -- stated in torch and run on the HIP kernels.

The statement.  Every row is its own search.  f: the classifier's logits [C]; x0 the image row (N
elements); t0 the first arg-max of f(x0); lo / hi the row's min / max unless ``bounds`` is given.  For logits s:
own = s[t0], other = the largest s[j], j != t0 (first on ties), A(s) = max(0, own - other + kappa), dA/ds = e_t0 - e_other
where own - other + kappa > 0 and 0 elsewhere.  An iterate v is a success when the first arg-max of f(v) is not t0.

The search on c: c = c0, c_lo = 0, c_hi = 1e10; ``binary_search_steps`` rounds, each from x0 with fresh optimiser state;
after a round with a success c_hi = min(c_hi, c), c = (c_lo + c_hi) / 2, after any other c_lo = max(c_lo, c) and
c = (c_lo + c_hi) / 2 if c_hi < 1e9 else 10 c.  The result is the best successful iterate of all rounds, its label and
found = 1, or x0 bit for bit, t0 and found = 0.

``cem_pn_statement`` is FISTA on (v, y), for k = 0 .. K-1:  g = c dA(f(y))/dy + 2 (y - x0), clipped to ``grad_clip`` in
the 2-norm;  u = y - learning_rate sqrt(1 - k / K) g;  w = min(u - beta, hi) / x0 / max(u + beta, lo) for u - x0 > beta
/ |u - x0| <= beta / u - x0 < -beta;  v' = w where w > x0 else x0;  y' = v' + k / (k + 3) (v' - v), then x0 where
y' <= x0.  Every v' is evaluated; the best is the success with the smallest |v' - x0|_2^2 + beta |v' - x0|_1.

``ce_statement`` is Adam (0.9 / 0.999 / 1e-8) on v:  g = c dA(f(v))/dv + gamma sign(v - x0), the same clip, the Adam
step, the clamp to [lo, hi].  Every updated v is evaluated; the best is the success with the smallest |v - x0|_1.

``cem_pp_statement`` is the pertinent positive (``'pp'``, what ``uncertainty_evolution.py`` reads) around a "no
information" pixel value b = ``background`` (fp32, default 0): the box of pixel i is [min(b, x0_i), max(b, x0_i)];
Apos(s) = max(0, other - own + kappa), dApos/ds = e_other - e_t0 where other - own + kappa > 0; a success is an
iterate whose first arg-max is t0.  With ``cem_pn_statement``'s hyper-parameters and v = y = b at the start of a round,
for k = 0 .. K-1:  g = c dApos(f(y))/dy + 2 (y - b), the same clip;  u = y - learning_rate sqrt(1 - k / K) g;
w = u - beta / b / u + beta for u - b > beta / |u - b| <= beta / u - b < -beta;  v' = w clamped to the box;
y' = v' + k / (k + 3) (v' - v) clamped to the box.  The best is the success with the smallest |v' - b|_2^2 +
beta |v' - b|_1; the c table and the unfound rows are as above (x0 is always a trivial positive).

What is stated is the published algorithm with omnixai's default hyper-parameters; agreement with the omnixai package
itself has not been checked (it is not a dependency).

``ContrastiveSearch`` is the device executor: the searches of a batch as replays of one HIP graph, no host read
inside.  CPU tensors and models that are no ``ClassifierStack`` run the statements.
"""
import math

import torch

from . import ops
from .graphs import GraphCache
from .pipeline import DecodeClassify, require_eval

PN_DEFAULTS = dict(c0=10.0, beta=0.1, kappa=10.0, binary_search_steps=5, learning_rate=1e-2, num_iterations=1000,
                   grad_clip=1e3)
CE_DEFAULTS = dict(c0=10.0, kappa=10.0, gamma=1.0, binary_search_steps=5, learning_rate=1e-2, num_iterations=100,
                   grad_clip=1e3)
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
C_HI0, C_HI_OPEN = 1e10, 1e9


def hyper_parameters(mode, hyper):
    """the mode's defaults with ``hyper`` on top; an unknown name is a ``TypeError``"""
    if mode not in ("pn", "ce"):
        raise ValueError(f"contrast: mode must be 'pn' or 'ce', got {mode!r}")
    out = dict(PN_DEFAULTS if mode == "pn" else CE_DEFAULTS)
    for k, v in hyper.items():
        if k not in out:
            raise TypeError(f"contrast: {k!r} is no hyper-parameter of mode {mode!r} ({sorted(out)})")
        out[k] = type(out[k])(v)
    if out["num_iterations"] < 1 or out["binary_search_steps"] < 1:
        raise ValueError("contrast: num_iterations and binary_search_steps must be at least 1")
    return out


# ---------------------------------------------------------------------- the statement, piece by piece (any dtype)
def attack_statement(s, t0, c, kappa):
    """(A [B], seed [B, C] = c * dA/ds, other [B]) of logits s [B, C], labels t0 [B] and constants c [B]"""
    B = s.shape[0]
    rows = torch.arange(B, device=s.device)
    t0 = t0.long()
    masked = s.clone()
    masked[rows, t0] = -math.inf
    other = masked.argmax(dim=1)                                  # (torch.argmax: the first maximum)
    margin = (s[rows, t0] - s[rows, other]) + kappa
    active = margin > 0
    seed = torch.zeros_like(s)
    seed[rows, t0] = 1
    seed[rows, other] = -1
    seed = seed * (c.to(s.dtype) * active.to(s.dtype)).unsqueeze(1)
    return torch.where(active, margin, torch.zeros_like(margin)), seed, other


def clip_statement(g, clip):
    """(g scaled to ``clip`` in the 2-norm where its norm is larger, the norm [B]) of g [B, N]"""
    norm = g.pow(2).sum(dim=1).sqrt()
    scale = torch.where(norm > clip, clip / norm, torch.ones_like(norm))
    return g * scale.unsqueeze(1), norm


def cem_update_statement(v, y, x0, gcls, k, K, lr, beta, clip, lo, hi):
    """One FISTA step: (v', y', l1, l2, norm) of v, y, x0 and gcls = c dA(f(y))/dy [B, N], lo / hi [B]"""
    lo, hi = lo.unsqueeze(1), hi.unsqueeze(1)
    g, norm = clip_statement(gcls + 2 * (y - x0), clip)
    u = y - lr * math.sqrt(1 - k / K) * g
    d = u - x0
    w = torch.where(d > beta, torch.minimum(u - beta, hi), torch.where(d < -beta, torch.maximum(u + beta, lo), x0))
    vn = torch.where(w > x0, w, x0)
    yn = vn + (k / (k + 3)) * (vn - v)
    yn = torch.where(yn > x0, yn, x0)
    diff = vn - x0
    return vn, yn, diff.abs().sum(dim=1), diff.pow(2).sum(dim=1), norm


def ce_update_statement(v, x0, gcls, m, v2, t, lr, gamma, clip, lo, hi, betas=ADAM_BETAS, eps=ADAM_EPS):
    """One Adam step (step count t >= 1): (v', m', v2', l1, norm) of v, x0, gcls = c dA(f(v))/dv, m, v2 [B, N]"""
    b1, b2 = betas
    g, norm = clip_statement(gcls + gamma * torch.sign(v - x0), clip)
    m = b1 * m + (1 - b1) * g
    v2 = b2 * v2 + (1 - b2) * g * g
    vn = v - (lr / (1 - b1 ** t)) * m / (v2.sqrt() / math.sqrt(1 - b2 ** t) + eps)
    vn = torch.minimum(torch.maximum(vn, lo.unsqueeze(1)), hi.unsqueeze(1))
    return vn, m, v2, (vn - x0).abs().sum(dim=1), norm


def attack_pp_statement(s, t0, c, kappa):
    """The pertinent-positive hinge: (Apos [B], seed [B, C] = c * dApos/ds, other [B]) of logits s [B, C], labels t0 [B]
    and constants c [B]; Apos = max(0, other - own + kappa), dApos/ds = e_other - e_t0 where that is > 0"""
    B = s.shape[0]
    rows = torch.arange(B, device=s.device)
    t0 = t0.long()
    masked = s.clone()
    masked[rows, t0] = -math.inf
    other = masked.argmax(dim=1)                                  # (torch.argmax: the first maximum)
    margin = (s[rows, other] - s[rows, t0]) + kappa
    active = margin > 0
    seed = torch.zeros_like(s)
    seed[rows, other] = 1
    seed[rows, t0] = -1
    seed = seed * (c.to(s.dtype) * active.to(s.dtype)).unsqueeze(1)
    return torch.where(active, margin, torch.zeros_like(margin)), seed, other


def pp_box(x0, background):
    """(lo, hi) [B, N]: per pixel min / max of the background and x0"""
    b = torch.full_like(x0, background)
    return torch.minimum(b, x0), torch.maximum(b, x0)


def pp_update_statement(v, y, x0, gcls, k, K, lr, beta, clip, background):
    """One FISTA step of the pertinent-positive search: (v', y', l1, l2, norm) of v, y, x0 and gcls = c dApos(f(y))/dy
    [B, N]; the shrink is centred on ``background`` (a float), the box is ``pp_box``, the distances are from the
    background"""
    lo, hi = pp_box(x0, background)
    b = torch.full_like(x0, background)
    g, norm = clip_statement(gcls + 2 * (y - b), clip)
    u = y - lr * math.sqrt(1 - k / K) * g
    d = u - b
    w = torch.where(d > beta, u - beta, torch.where(d < -beta, u + beta, b))
    vn = torch.minimum(torch.maximum(w, lo), hi)
    yn = vn + (k / (k + 3)) * (vn - v)
    yn = torch.minimum(torch.maximum(yn, lo), hi)
    diff = vn - b
    return vn, yn, diff.abs().sum(dim=1), diff.pow(2).sum(dim=1), norm


def c_table_statement(c, c_lo, c_hi, success):
    """The binary search on c after a round: (c, c_lo, c_hi) [B] of the same and ``success`` [B] bool"""
    hi_s = torch.minimum(c_hi, c)
    lo_f = torch.maximum(c_lo, c)
    c_f = torch.where(c_hi < C_HI_OPEN, (lo_f + c_hi) / 2, c * 10)
    return (torch.where(success, (c_lo + hi_s) / 2, c_f), torch.where(success, c_lo, lo_f),
            torch.where(success, hi_s, c_hi))


def row_bounds(x0, bounds):
    """(lo [B], hi [B]) in the dtype of x0 [B, N]"""
    if bounds is None:
        return x0.amin(dim=1), x0.amax(dim=1)
    lo, hi = bounds
    return torch.full_like(x0[:, 0], float(lo)), torch.full_like(x0[:, 0], float(hi))


def class_gradient(f, point, t0, c, kappa, attack=attack_statement):
    """c * dA(f(point))/dpoint in the shape of ``point`` (autograd through ``f``; ``attack``: the hinge's statement,
    ``attack_pp_statement`` for pertinent positives)"""
    with torch.enable_grad():
        p = point.detach().requires_grad_(True)
        s = f(p)
        _, seed, _ = attack(s.detach(), t0, c, kappa)
        g, = torch.autograd.grad(s, p, seed)
    return g.detach()


def as_fp32(value):
    """a Python float that is an fp32 value: the background as the kernels take it"""
    return float(torch.tensor(float(value), dtype=torch.float32))


def _search(f, x, mode, hp, bounds, record, background=None):
    x = x.detach()
    B, shape = x.shape[0], x.shape
    x0 = x.reshape(B, -1)
    K, rounds = hp["num_iterations"], hp["binary_search_steps"]
    fista = mode in ("pn", "pp")
    with torch.no_grad():
        t0 = f(x).argmax(dim=1)
    lo, hi = row_bounds(x0, bounds)
    c = torch.full_like(lo, hp["c0"])
    c_lo, c_hi = torch.zeros_like(lo), torch.full_like(lo, C_HI0)
    best, best_dist = x0.clone(), torch.full_like(lo, math.inf)
    best_label, found = t0.clone(), torch.zeros(B, dtype=torch.bool, device=x.device)
    for r in range(rounds):
        if mode == "pp":
            v, y = torch.full_like(x0, background), torch.full_like(x0, background)
        else:
            v, y = x0.clone(), x0.clone()
        m, v2 = torch.zeros_like(x0), torch.zeros_like(x0)
        round_succ = torch.zeros(B, dtype=torch.bool, device=x.device)
        for k in range(K):
            gcls = class_gradient(f, (y if fista else v).reshape(shape), t0, c, hp["kappa"],
                                  attack_pp_statement if mode == "pp" else attack_statement).reshape(B, -1)
            if mode == "pn":
                v, y, l1, l2, _ = cem_update_statement(v, y, x0, gcls, k, K, hp["learning_rate"], hp["beta"],
                                                       hp["grad_clip"], lo, hi)
                dist = l2 + hp["beta"] * l1
            elif mode == "pp":
                v, y, l1, l2, _ = pp_update_statement(v, y, x0, gcls, k, K, hp["learning_rate"], hp["beta"],
                                                      hp["grad_clip"], background)
                dist = l2 + hp["beta"] * l1
            else:
                v, m, v2, dist, _ = ce_update_statement(v, x0, gcls, m, v2, k + 1, hp["learning_rate"], hp["gamma"],
                                                        hp["grad_clip"], lo, hi)
            with torch.no_grad():
                pred = f(v.reshape(shape)).argmax(dim=1)
            succ = pred == t0 if mode == "pp" else pred != t0
            better = succ & (dist < best_dist)
            best = torch.where(better.unsqueeze(1), v, best)
            best_dist = torch.where(better, dist, best_dist)
            best_label = torch.where(better, pred, best_label)
            found |= better
            round_succ |= succ
            if record is not None:
                record.append(dict(round=r, k=k, c=c.clone(), v=v.clone(), pred=pred.clone(), succ=succ.clone(),
                                   dist=dist.clone()))
        c, c_lo, c_hi = c_table_statement(c, c_lo, c_hi, round_succ)
    return {"image": best.reshape(shape), "label": best_label.to(torch.int32), "found": found.to(torch.int32),
            "dist": torch.where(found, best_dist, torch.zeros_like(best_dist)), "c": c}


def cem_pn_statement(f, x, bounds=None, record=None, **hyper):
    """Pertinent negatives of x [B, ...] under the logits ``f`` (module docstring), in the dtype of x.  Returns
    {"image", "label" int32, "found" int32, "dist" (of the returned image: 0 where nothing was found), "c" (after the
    last round)}.  ``record``: a list that receives every evaluated iterate."""
    return _search(f, x, "pn", hyper_parameters("pn", hyper), bounds, record)


def ce_statement(f, x, bounds=None, record=None, **hyper):
    """Counterfactuals of x [B, ...] under the logits ``f`` (module docstring); returns what ``cem_pn_statement`` does"""
    return _search(f, x, "ce", hyper_parameters("ce", hyper), bounds, record)


def cem_pp_statement(f, x, background=0.0, record=None, **hyper):
    """Pertinent positives of x [B, ...] under the logits ``f`` around the "no information" value ``background`` (an
    fp32 scalar; module docstring), with the hyper-parameters and defaults of ``cem_pn_statement``; returns what
    ``cem_pn_statement`` does, ``dist`` measured from the background."""
    return _search(f, x, "pp", hyper_parameters("pn", hyper), None, record, as_fp32(background))


# ---------------------------------------------------------------------- the device executor
class ContrastiveSearch:
    """``run(x [B,1,H,W] cuda)`` -> {"image" [B,1,H,W], "label" [B] int32, "found" [B] int32, "dist" [B], "c" [B]} on the
    device, without a host read: ``mode`` "pn" is ``cem_pn_statement``, "ce" is ``ce_statement``, "pp" is
    ``cem_pp_statement`` around ``background`` (default 0.0; "pp" only), B rows as B searches.

    One replay of the recorded graph at iteration counter k (device memory, per row) is: the classifier's forward chain
    over the iterates v_k (and, "pn" / "pp", the slack rows y_k behind them: one chain call of 2B rows),
    ``ali_ct_attack`` (``ali_ct_pp_attack`` in "pp"; evaluation of v_k, seed at the gradient point), ``ali_ct_book``
    (best so far; at k == K the move of c), the chain's data-gradient pass over the gradient point's rows
    (``need_params=False``: no parameter or ``.grad`` is touched) and the mode's update kernel (k < K: the step to
    v_(k+1); k == K: the next round starts from x0, in "pp" from the background).  A round is K + 1 replays, a search
    ``binary_search_steps`` * (K + 1); the graph is recorded once per (B, H, W, mode, hyper-parameters, bounds,
    background, module mode).

    The classifier must be a ``ClassifierStack`` (``TypeError`` otherwise) in eval mode and, for "pn" and "pp", without
    BatchNorm layers (``ValueError``: the slack rows' gradient is taken from a 2B-row pass); CPU tensors are refused
    (the statements serve them), and so are ``bounds`` in "pp" and ``background`` in "pn" / "ce" (``ValueError``).  t0 is
    the first arg-max of the logits of x0 in a pass of the batch shape the replays use (2B rows for "pn" / "pp", B for
    "ce").  ``start`` / ``advance`` / ``result`` are ``run`` in pieces (tests, inspection)."""

    def __init__(self, classifier, mode="pn", capture=True, bounds=None, background=None, **hyper):
        self.pipe = DecodeClassify(classifier)
        self.classifier, self.mode, self.capture = classifier, mode, capture
        self.hp = hyper_parameters("pn" if mode == "pp" else mode, hyper)
        if mode == "pp":
            if bounds is not None:
                raise ValueError("ContrastiveSearch: mode 'pp' takes its box from x0 and the background; bounds are "
                                 "for 'pn' / 'ce'")
            background = as_fp32(0.0 if background is None else background)
        elif background is not None:
            raise ValueError(f"ContrastiveSearch: background belongs to mode 'pp', not {mode!r}")
        self.background = background
        self.bounds = None if bounds is None else (float(bounds[0]), float(bounds[1]))
        self._check_eval()
        if mode in ("pn", "pp") and any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
                                        for m in classifier.modules()):
            raise ValueError(f"ContrastiveSearch: mode {mode!r} takes the data gradient over the slack rows of a 2B-row "
                             "forward pass, which needs a classifier without BatchNorm layers")
        self._graphs = GraphCache(modules=[classifier])
        self._state = {}
        self._cur = None

    def _check_eval(self):
        require_eval("ContrastiveSearch", classifier=self.classifier)

    @property
    def replays_per_search(self):
        return self.hp["binary_search_steps"] * (self.hp["num_iterations"] + 1)

    def _buffers(self, B, H, W, device):
        key = (B, H, W, str(device))
        st = self._state.get(key)
        if st is None:
            N, R = H * W, (2 * B if self.mode in ("pn", "pp") else B)
            f = dict(dtype=torch.float32, device=device)
            i = dict(dtype=torch.int32, device=device)
            st = self._state[key] = dict(
                rows=torch.zeros(R, 1, H, W, **f), x0=torch.zeros(B, N, **f), lo=torch.zeros(B, **f),
                hi=torch.zeros(B, **f), t0=torch.zeros(B, **i), ctab=torch.zeros(3, B, **f), it=torch.zeros(B, **i),
                rnd=torch.zeros(B, **i), dist=torch.zeros(B, **f), l1=torch.zeros(B, **f), l2=torch.zeros(B, **f),
                gnorm=torch.zeros(B, **f), best=torch.zeros(B, N, **f), best_dist=torch.zeros(B, **f),
                best_label=torch.zeros(B, **i), found=torch.zeros(B, **i), round_succ=torch.zeros(B, **i),
                copied=torch.zeros(B, **i))
            if self.mode == "ce":
                st["m"], st["v2"] = torch.zeros(B, N, **f), torch.zeros(B, N, **f)
            st["key"], st["B"], st["N"] = key, B, N
        return st

    def _mutable(self, st):
        names = ["rows", "ctab", "it", "rnd", "dist", "l1", "l2", "gnorm", "best", "best_dist", "best_label", "found",
                 "round_succ", "copied"] + (["m", "v2"] if self.mode == "ce" else [])
        return [st[n] for n in names]

    # ---- what the graph records: one replay
    def _iter(self, st, x0, lo, hi, t0):
        B, N, hp, pp = st["B"], st["N"], self.hp, self.mode == "pp"
        fista = self.mode in ("pn", "pp")
        rows = st["rows"]
        R = rows.shape[0]
        lg, saved = self.pipe.classify(rows, save=True)
        flat = rows.reshape(R, N)
        v = flat[:B]
        attack = ops.ct_pp_attack if pp else ops.ct_attack
        seed, A, pred, succ = attack(lg, B, t0, st["ctab"][0], hp["kappa"], 0, B if fista else 0)
        dist = st["dist"] if fista else st["l1"]
        ops.ct_book(v, dist, succ, pred, st["it"], hp["num_iterations"], st["best"], st["best_dist"], st["best_label"],
                    st["found"], st["round_succ"], st["ctab"], st["copied"])
        # "pn" / "pp": the slack rows alone -- rows of a stack without BatchNorm are independent
        gx = self.pipe.image_grad(saved, seed, rows=(B, 2 * B) if fista else None)
        if pp:
            ops.ct_pp_update(gx, v, flat[B:], x0, self.background, st["it"], st["rnd"], hp["num_iterations"],
                             hp["learning_rate"], hp["beta"], hp["grad_clip"], st["l1"], st["l2"], st["dist"],
                             st["gnorm"])
        elif fista:
            ops.ct_cem_update(gx, v, flat[B:], x0, lo, hi, st["it"], st["rnd"], hp["num_iterations"],
                              hp["learning_rate"], hp["beta"], hp["grad_clip"], st["l1"], st["l2"], st["dist"],
                              st["gnorm"])
        else:
            ops.ct_ce_update(gx, v, x0, lo, hi, st["m"], st["v2"], st["it"], st["rnd"], hp["num_iterations"],
                             hp["learning_rate"], hp["gamma"], hp["grad_clip"], st["l1"], st["gnorm"], ADAM_BETAS,
                             ADAM_EPS)
        st["probe"] = {"logits": lg, "seed": seed, "A": A, "pred": pred, "succ": succ, "gx": gx}   # (tests, inspection)
        return pred

    # ---- run, in pieces
    @torch.no_grad()
    def start(self, x):
        """Puts the searches of x [B,1,H,W] at the start of their first round; returns the state (device tensors)."""
        self._check_eval()
        if not (torch.is_tensor(x) and x.is_cuda):
            raise ValueError("ContrastiveSearch: needs CUDA tensors (CPU tensors: cem_pn_statement / ce_statement)")
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"ContrastiveSearch: need images [B, 1, H, W], got {tuple(x.shape)}")
        B, _, H, W = x.shape
        st = self._buffers(B, H, W, x.device)
        st["x0"].copy_(x.detach().reshape(B, -1).float())
        x0 = st["x0"]
        lo, hi = row_bounds(x0, self.bounds)
        st["lo"].copy_(lo)
        st["hi"].copy_(hi)
        rows = st["rows"]
        R = rows.shape[0]
        rows.copy_(x0.reshape(B, 1, H, W).repeat(R // B, 1, 1, 1))
        # t0 from a pass of the batch shape the replays evaluate their iterates in: a row's logits depend on the
        # batch size in the last bits, and an iterate still at x0 must not count as a success by rounding alone
        logits, _ = self.pipe.classify(rows, save=True)                                          # (as a replay's)
        _, _, t0, _ = ops.ct_attack(logits, B)
        st["t0"].copy_(t0)
        if self.mode == "pp":                                       # the iterates start from the background
            rows.fill_(self.background)
        st["ctab"][0].fill_(self.hp["c0"])
        st["ctab"][1].zero_()
        st["ctab"][2].fill_(C_HI0)
        st["best"].copy_(x0)
        st["best_dist"].fill_(math.inf)
        st["best_label"].copy_(st["t0"])
        for n in ["it", "rnd", "dist", "l1", "l2", "gnorm", "found", "round_succ", "copied"] + \
                (["m", "v2"] if self.mode == "ce" else []):
            st[n].zero_()
        self._cur = st
        return st

    @torch.no_grad()
    def advance(self, n=1):
        """``n`` replays on the searches ``start`` set up"""
        st = self._cur
        if st is None:
            raise RuntimeError("ContrastiveSearch.advance: call start(x) first")
        self._check_eval()
        args = (st["x0"], st["lo"], st["hi"], st["t0"])
        if n < 1:
            return
        if not self.capture:
            for _ in range(n):
                self._iter(st, *args)
            return
        extra = (st["key"], self.mode, tuple(sorted(self.hp.items())), self.bounds, self.background,
                 self.classifier.training)
        self._graphs(lambda *a: self._iter(st, *a), args, extra, self._mutable(st))
        self._graphs.replay(args, extra, n - 1)                           # the inputs are in place: replay only

    @torch.no_grad()
    def result(self):
        st = self._cur
        B = st["B"]
        found = st["found"].clone()
        return {"image": st["best"].reshape((B,) + tuple(st["rows"].shape[1:])).clone(), "label": st["best_label"].clone(),
                "found": found, "dist": torch.where(found != 0, st["best_dist"], torch.zeros_like(st["best_dist"])),
                "c": st["ctab"][0].clone()}

    def run(self, x):
        self.start(x)
        self.advance(self.replays_per_search)
        return self.result()
