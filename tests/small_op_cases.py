"""Case lists, input builders, fp64 references and bounds of the small-op tests: dense Adam (ops.adam_step /
ops.adam_step_at), the hidden-layer dropout (ops.dropout_hidden / functional.dropout_hidden) and the index check
(ops.check_indices), all of csrc/misc.hip.  test_gpu_small_ops.py runs them on the GPU, test_small_op_bounds_host.py
checks on the CPU that the lists cover what they claim, that the Adam bound cannot reject a correct kernel and that
the data can tell a subtly wrong one from a right one.  Pure torch / numpy: importable without a GPU; the reference and
the bound are torch expressions, so they run on whichever device their inputs live on.

THE ADAM BOUND (adam_bound).  Every comparison is ONE step from a given fp32 state (p, m, v, g, t) against torch's
single-tensor Adam evaluated in fp64 with the exact double hyper-parameters (adam_ref).  Write u = 2^-24.  Every fp32
operation of pc_adam_update (common.h) and every constant it rounds to fp32 is allowed one ulp, i.e. a relative 2u
(a correctly rounded operation uses half of that), and 2^-149 where its result is an fp32 subnormal:

    m' = m + (g - m) * omb1             subtraction, omb1 = fl(1 - beta1), product: 3 x 2u on omb1 |g - m| <= |m| + |g|;
                                        the sum: 2u |m'| <= 2u (|m| + |g|)
          err_m = CM u (|m| + |g|) + 3 SUB,   CM = 8
    v' = v * beta2 + (omb2 * g) * g     both terms are >= 0; the longer chain (omb2 = fl(1 - beta2), two products) and the
                                        sum: 4 x 2u on at most v'
          err_v = CV u v' + 3 SUB,            CV = 8
    den = sqrt(v') / bc2s + eps         what err_v does to the root: |sqrt a - sqrt b| <= sqrt|a - b| always, and
                                        <= |a - b| / 2 sqrt b to first order
          err_den = min(sqrt err_v, err_v / 2 sqrt v') / bc2s
    p' = p - step_size * (m' / den)     the root, bc2s = fl(sqrt(1 - beta2^t)), the division by it, eps = fl(eps), the
                                        sum, the quotient, step_size = fl(lr / (1 - beta1^t)), the product: 8 x 2u, each on
                                        a factor of the update D = ss m' / den; the final subtraction: 2u |p'|
          err_p = ss err_m / den + |D| err_den / den + CD u |D| + CP u |p'| + 3 SUB,   CD = 16, CP = 2

(ss, den, D: the fp64 step size, denominator and update.)  The coefficients are these operation counts and nothing else:
no GPU result went into them.  What two correct evaluations make of the bound, worst element over every family below,
both p modes, t in ADAM_STEPS, both hyper-parameter sets, n = 65537 (test_small_op_bounds_host.py prints and asserts
them):

    RECORDED RATIOS (error / bound)                        p        m        v
      adam_restate (the kernel's arithmetic, numpy fp32)   0.499    0.120    0.334     p ~ N(0,1)
                                                           0.175    0.119    0.333     p = 0
      torch.optim.Adam, fp32 on the CPU                    0.499    0.120    0.334     p ~ N(0,1)
                                                           0.179    0.120    0.333     p = 0

(0.5 on p is the final subtraction's half ulp against the whole ulp it is allowed; with p = 0 the update itself is
judged.  torch forms (value m) / den in another order.)
Deliberately wrong restatements miss the same bound -- worst element of p' over the named family at p = 0, n = 4099:

    RECORDED MISS FACTORS (error / bound, asserted >= 2; the right form on the same data: <= 0.15)
      eps inside the correction, (sqrt v + eps) / bc2s      near_eps, t = 1000, defaults        6.9e4
                                                            near_eps, t = 1,    defaults        3.1e5
      fp32 powf bias corrections from fp32 betas            train,    t = 1,    defaults        3.7
                                                            train,    t = 2,    defaults        5.5
      step number t + 1                                     train,    t = 1,    defaults        1.4e5
                                                            first,    t = 1,    second set      8.0e4
      skipping on g == 0 alone                              g0_live,  t = 1000, defaults        5.4e5
"""
import functools

import numpy as np
import torch

from oracle import philox_oracle

U = 2.0 ** -24              # fp32 unit roundoff: half an ulp, relative
SUB = 2.0 ** -149           # the smallest fp32 subnormal: one ulp down there

# ====================================================================================== Adam
# (6: a two-element tail behind a float4 group, the one residue the issue's list has only without a group in front)
ADAM_SIZES = (1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1025, 1027, 4099, 65537)
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_HYPER = ((1e-3, 0.9, 0.999, 1e-8), (3e-2, 0.5, 0.9, 1e-6))          # (lr, beta1, beta2, eps)
ADAM_FAMILIES = ("train", "near_eps", "tiny", "wide", "first", "g0_live", "dead_mix")
P_MODES = ("normal", "zero")
# `tiny` moves p by 1e-17: next to p ~ N(0,1) nothing of it is left to judge
ADAM_FAMILY_MODES = [(f, pm) for f in ADAM_FAMILIES for pm in P_MODES if not (f == "tiny" and pm == "normal")]
CM, CV, CD, CP = 8.0, 8.0, 16.0, 2.0
ADAM_BLOCK = 256            # threads per workgroup of adam_kernel / adam_at_kernel, four elements per thread


def adam_launch(n):
    """(workgroups, elements of the scalar tail, threads of the last workgroup) of both Adam kernels at size n"""
    threads = (n + 3) // 4
    return (threads + ADAM_BLOCK - 1) // ADAM_BLOCK, n % 4, (threads - 1) % ADAM_BLOCK + 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def adam_inputs(family, p_mode, n, seed=0):
    """fp32 CPU tensors (p, m, v, g) of one family; v >= 0 (or -0.0 in dead groups)"""
    gen = _gen(7000 + 131 * ADAM_FAMILIES.index(family) + seed)
    randn = lambda: torch.randn(n, generator=gen)
    spread = lambda: 0.5 + torch.rand(n, generator=gen)
    p = randn() if p_mode == "normal" else torch.zeros(n)
    if family == "train":
        g, m, v = 1e-2 * randn(), 1e-2 * randn(), 1e-4 * spread()
    elif family == "near_eps":          # sqrt(v) / bc2s ~ 1e-8 .. 3e-7: eps (1e-8 / 1e-6) decides the denominator with it
        g, m, v = 1e-8 * randn(), 1e-8 * randn(), 1e-16 * spread()
    elif family == "tiny":              # g^2 ~ 1e-44 and v: a handful of subnormal units
        g, m, v = 1e-22 * randn(), 1e-22 * randn(), 1e-44 * spread()
    elif family == "wide":              # nine decades of per-element scale
        s = 10.0 ** (-6.0 + 9.0 * torch.rand(n, generator=gen))
        g, m, v = s * randn(), s * randn(), s * s * spread()
    elif family == "first":
        g, m, v = 1e-2 * randn(), torch.zeros(n), torch.zeros(n)
    elif family == "g0_live":
        g, m, v = torch.zeros(n), 1e-2 * randn(), 1e-4 * spread()
    elif family == "dead_mix":
        gl, ml, vl = 1e-2 * randn(), 1e-2 * randn(), 1e-4 * spread()
        g, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
        for k in range(n // 4):
            if k % 2 == 0:              # dead: twelve zeros, every other one with negative zeros among them
                if k % 4 == 0:
                    v[4 * k], m[4 * k + 1], g[4 * k + 2] = -0.0, -0.0, -0.0
                    if p_mode == "zero":
                        p[4 * k + 3] = -0.0
            else:                       # exactly one of the twelve values is non-zero; its place walks through all twelve
                which, lane = divmod((k // 2) % 12, 4)
                (g, m, v)[which][4 * k + lane] = (gl, ml, vl)[which][4 * k + lane]
        tail = slice(n - n % 4, n)      # the scalar tail has no skip: live values
        g[tail], m[tail], v[tail] = gl[tail], ml[tail], vl[tail]
    else:
        raise ValueError(family)
    return p.float(), m.float(), v.float(), g.float()


def dead_elements(m, v, g):
    """bool [n]: elements of COMPLETE float4 groups whose twelve values are all zero (of either sign) -- what
    pc_adam_dead skips.  The tail is never dead."""
    n = g.numel()
    full = n - n % 4
    z = ((g[:full] == 0) & (m[:full] == 0) & (v[:full] == 0)).view(-1, 4).all(1)
    out = torch.zeros(n, dtype=torch.bool, device=g.device)
    out[:full] = z.repeat_interleave(4)
    return out


def adam_scalars(t, hyper):
    """torch's single-tensor path: python doubles"""
    lr, b1, b2, eps = hyper
    return lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5


def adam_ref(p, m, v, g, t, hyper):
    """One step of torch.optim.Adam's single-tensor update in fp64 from the fp32 state: dict of fp64 tensors"""
    lr, b1, b2, eps = hyper
    ss, bc2s = adam_scalars(t, hyper)
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    m1 = m + (g - m) * (1.0 - b1)                         # exp_avg.lerp_(grad, 1 - beta1)
    v1 = v * b2 + (1.0 - b2) * g * g                      # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    den = v1.sqrt() / bc2s + eps
    delta = ss * (m1 / den)
    return {"p": p - delta, "m": m1, "v": v1, "den": den, "delta": delta, "ss": ss, "bc2s": bc2s}


def adam_bound(p, m, v, g, t, hyper, ref=None):
    """(err_p, err_m, err_v): per-element fp64 bounds, derived in the module docstring"""
    r = ref if ref is not None else adam_ref(p, m, v, g, t, hyper)
    err_m = CM * U * (m.double().abs() + g.double().abs()) + 3 * SUB
    err_v = CV * U * r["v"].abs() + 3 * SUB
    root = r["v"].abs().sqrt()
    first_order = torch.where(root > 0, err_v / (2 * root.clamp_min(1e-300)), torch.full_like(root, float("inf")))
    err_den = torch.minimum(err_v.sqrt(), first_order) / r["bc2s"]
    d = r["delta"].abs()
    err_p = r["ss"] * err_m / r["den"] + d * err_den / r["den"] + CD * U * d + CP * U * r["p"].abs() + 3 * SUB
    return err_p, err_m, err_v


def adam_ratios(got_p, got_m, got_v, p, m, v, g, t, hyper):
    """worst error / bound of (p, m, v) against the fp64 reference of one step from (p, m, v, g)"""
    r = adam_ref(p, m, v, g, t, hyper)
    bounds = adam_bound(p, m, v, g, t, hyper, ref=r)
    out = []
    for got, want, b in zip((got_p, got_m, got_v), (r["p"], r["m"], r["v"]), bounds):
        if not bool(torch.isfinite(got).all()):
            out.append(float("inf"))
        else:
            out.append(float(((got.double() - want).abs() / b).max()))
    return tuple(out)


ADAM_FORMS = ("kernel", "eps_inside", "powf32", "t_plus_1", "skip_g0")


def adam_restate(p, m, v, g, t, hyper, form="kernel"):
    """The arithmetic of adam_prep_kernel + pc_adam_update in numpy fp32, one rounding per operation, no contraction
    (form "kernel"), and four deliberately wrong variants.  Returns fp32 torch tensors (p', m', v')."""
    f = np.float32
    lr, b1, b2, eps = hyper
    p, m, v, g = (x.numpy().astype(f) for x in (p, m, v, g))
    tt = t + 1 if form == "t_plus_1" else t
    if form == "powf32":                # the corrections formed in fp32 from fp32 betas
        bc1 = f(1) - np.power(f(b1), f(tt), dtype=f)
        bc2 = f(1) - np.power(f(b2), f(tt), dtype=f)
        ss, bc2s = f(lr) / bc1, np.sqrt(bc2, dtype=f)
    else:
        ss, bc2s = (f(x) for x in adam_scalars(tt, hyper))
    omb1, beta2, omb2, epsf = f(1.0 - b1), f(b2), f(1.0 - b2), f(eps)
    with np.errstate(all="ignore"):
        m1 = m + (g - m) * omb1
        v1 = v * beta2 + (omb2 * g) * g
        den = (np.sqrt(v1) + epsf) / bc2s if form == "eps_inside" else np.sqrt(v1) / bc2s + epsf
        p1 = p - ss * (m1 / den)
    if form == "skip_g0":
        keep = g == 0
        p1, m1, v1 = np.where(keep, p, p1), np.where(keep, m, m1), np.where(keep, v, v1)
    return tuple(torch.from_numpy(np.ascontiguousarray(x.astype(f))) for x in (p1, m1, v1))


def adam_torch_fp(p, m, v, g, t, hyper, dtype=torch.float32):
    """One step of torch.optim.Adam itself (single-tensor path, CPU) from the given state, in `dtype`"""
    lr, b1, b2, eps = hyper
    w = p.detach().cpu().to(dtype).clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(t - 1)), "exp_avg": m.cpu().to(dtype).clone(),
                    "exp_avg_sq": v.cpu().to(dtype).clone()}
    w.grad = g.cpu().to(dtype).clone()
    opt.step()
    st = opt.state[w]
    assert int(st["step"]) == t
    return w.detach(), st["exp_avg"], st["exp_avg_sq"]


# ====================================================================================== hidden dropout
DROP_SIZES = (4, 8, 1020, 1024, 1028, 4 * 4099)
DROP_PROBS = (0.1, 0.5, 0.25, 1e-10, 1.0 - 2.0 ** -20)
DROP_SEEDS = (4242, (1 << 32) + 77)                 # below and above 2^32
DROP_OFFSETS = (6, (5 << 32) + 3)
DROP_REFUSED_P = (0.0, -0.1, 1.0, 1.5, 1.0 - 2.0 ** -30, 1e-50)   # the last two round to 1.0f and 0.0f
DROP_REFUSED_N = (1, 2, 3, 5, 1023)
DROP_MAX_GROUPS = 20000                             # the oracle is a pure-Python loop over groups of four


@functools.lru_cache(maxsize=None)
def _mask(seed, offset, n, p):
    assert (n + 3) // 4 <= DROP_MAX_GROUPS
    out = philox_oracle.dropout_mask(seed, offset, philox_oracle.STREAM_HIDDEN, n, p)
    out.setflags(write=False)
    return out


def hidden_mask(seed, offset, n, p):
    """philox_oracle.dropout_mask(seed, offset, STREAM_HIDDEN, n, p): fp32 [n], computed once per argument set, read-only"""
    return _mask(int(seed), int(offset), int(n), float(p))


def drop_input(n, seed=0):
    """N(0,1) with both zeros and a value whose product with 2^20 is still finite"""
    x = torch.randn(n, generator=_gen(8000 + seed))
    x[0], x[n - 1] = -0.0, 0.0
    if n > 4:
        x[2] = -3.5
    return x


def drop_expected(x, mask):
    """x * mask in fp32 (numpy): a dropped negative value is -0.0, as in the kernel's single product"""
    return torch.from_numpy(x.numpy().astype(np.float32) * mask)


# ====================================================================================== index check
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
IDX_LENGTHS = (1, 255, 256, 257, 4099)
IDX_HIS = (1, 7, 1000, I32_MAX)
IDX_SPECIALS = ("m2", "m1", "zero", "hi_m1", "hi", "min", "max")
IDX_PLACES = ("first", "last", "before_256", "at_256")
IDX_BLOCK = 256
IDX_ROTATIONS = 14


def idx_special(name, hi):
    return {"m2": -2, "m1": -1, "zero": 0, "hi_m1": hi - 1, "hi": hi, "min": I32_MIN, "max": I32_MAX}[name]


def idx_places(n):
    """{place: position} of an array of n entries: the first and last element, each side of the 256-element boundary"""
    out = {"first": 0, "last": n - 1}
    if n > IDX_BLOCK:
        out["before_256"], out["at_256"] = IDX_BLOCK - 1, IDX_BLOCK
    return out


def idx_case(count, rot):
    """`count` arrays of unequal lengths: list of (int32 numpy array, hi, allow_pad, {place: special name})"""
    rng = np.random.default_rng(9000 + 100 * count + rot)
    jobs = []
    for a in range(count):
        n = IDX_LENGTHS[(rot + 2 * a + count) % len(IDX_LENGTHS)]      # (step 2 mod 5: distinct lengths, longest anywhere)
        hi = IDX_HIS[(rot + a) % len(IDX_HIS)]
        allow_pad = bool(((rot // 7) + a) % 2)
        arr = rng.integers(0, hi, size=n, dtype=np.int64)
        at = {}                                                         # (n = 1, 256, 257: two places are one position)
        for k, place in enumerate(p for p in IDX_PLACES if p in idx_places(n)):
            at[idx_places(n)[place]] = IDX_SPECIALS[(rot + 3 * a + k) % len(IDX_SPECIALS)]
        for pos, name in at.items():
            arr[pos] = idx_special(name, hi)
        planted = {place: at[pos] for place, pos in idx_places(n).items()}
        if n > 300:                                                     # some more bad and pad entries anywhere
            for pos in rng.integers(1, n - 1, size=6):
                if pos not in (IDX_BLOCK - 1, IDX_BLOCK):
                    arr[pos] = rng.choice([-1, -1, hi, -7, hi - 1])
        jobs.append((arr.astype(np.int32), hi, allow_pad, planted))
    return jobs


def idx_bad_count(jobs):
    """the exact number of entries check_indices must add: outside [0, hi), a -1 excused where allow_pad is set"""
    total = 0
    for arr, hi, allow_pad, _ in jobs:
        a = arr.astype(np.int64)
        total += int(np.count_nonzero((a >= hi) | (a < (-1 if allow_pad else 0))))
    return total


def idx_legal_case(count):
    rng = np.random.default_rng(9900 + count)
    jobs = []
    for a in range(count):
        n, hi, allow_pad = IDX_LENGTHS[(a + 1) % len(IDX_LENGTHS)], IDX_HIS[(a + 1) % len(IDX_HIS)], a % 2 == 0
        arr = rng.integers(0, hi, size=n, dtype=np.int64)
        arr[0], arr[n - 1] = (-1 if allow_pad else 0), hi - 1
        jobs.append((arr.astype(np.int32), hi, allow_pad, {}))
    return jobs
