"""The view fold's eligibility decision (nerf-projects_amd/csrc/refresh_kernels.hip, view_fold_eligible_kernel) restated on
the host in fp64 numpy, and the networks tests/test_view_fold.py and tests/test_view_fold_cpu.py hold it against.

fold_rule works from the state dict as loaded. The device applies the same three rules to the ROW-EQUALISED copy
(mlp_kernel_h2.hip, row_exponents_kernel: unit j of a layer is scaled by 2^e_j, e_j = median binade of the layer's row norms
minus the row's own, |e_j| <= 30, and column j of its consumer by 2^-e_j), so the two can differ:
  * the feature units' factors cancel in W_vf = W_v[:, :W] W_f;
  * a view row's factor multiplies both column blocks of that row: the two blocks' maxima move apart only when they sit in
    different rows, by at most max e - min e over the view rows;
  * feature_linear's rows take their own factor and its columns the inverse of the last trunk layer's.
A layer whose rows are of like size (norms within a factor of two of each other, as every layer of the networks named here
is: uniform initialisation, and every scaling below multiplies whole tensors or whole column blocks) spreads over at most
three adjacent binades around its median, so |e_j| <= 1: the ratio moves by at most 2^2 and the gain by at most 2^2 (one
for the rows, one for the columns). The verdict leaves 2^3 and 2^4. equalised_rule restates the device's side - the
exponents as row_exponents_kernel chooses them, then the rule on the scaled copy - and tests/test_view_fold_cpu.py checks, for
every network named here, that the movement is inside the slack and that the device's decision is the verdict's."""
from collections import OrderedDict

import numpy as np

from nerf_projects_amd import synthetic

GAIN_LIMIT, GAIN_SLACK = 128, 4          # gain 2^64 + bmax must stay finite: below 2^128
RATIO_LIMIT, RATIO_SLACK = 8, 3          # the two column blocks of the folded layer within 2^8


def arch_of(D=8, W=256, skips=(4,), input_ch=63, input_ch_views=27):
    return dict(D=D, W=W, skips=tuple(skips), input_ch=input_ch, input_ch_views=input_ch_views)


BENCH = arch_of()


def net_kwargs(arch):
    """make_net's keywords for an arch of this module."""
    return dict(D=arch["D"], W=arch["W"], skips=list(arch["skips"]), input_ch=arch["input_ch"],
                input_ch_views=arch["input_ch_views"], use_viewdirs=True, output_ch=4)


def _f64(sd, key):
    return np.asarray(sd[key], dtype=np.float64)


def _finite32(*arrays):
    with np.errstate(over="ignore", invalid="ignore"):
        return all(np.isfinite(a.astype(np.float32)).all() for a in arrays)


def _rule(wf, bf, wv, bv, W):
    """(finite, g, r) of one set of matrices."""
    with np.errstate(over="ignore", invalid="ignore"):
        w_vf = wv[:, :W] @ wf
        b_vf = wv[:, :W] @ bf + bv
    finite = _finite32(wf, bf, wv, bv, w_vf, b_vf)
    if not finite:
        return False, None, None
    g = float(np.log2(np.abs(wf).sum(1).max() * 2.0 ** 64 + np.abs(bf).max()))
    m_vf, m_d = np.abs(w_vf).max(), (np.abs(wv[:, W:]).max() if wv.shape[1] > W else 0.0)
    r = float(np.log2(m_vf / m_d)) if (m_vf > 0 and m_d > 0) else None
    return True, g, r


def fold_rule(sd, arch):
    """(finite, g, r) from the state dict as loaded: whether every entry of W_f, b_f, W_v, b_v, W_vf and b_vf is finite
    in fp32; g = log2(largest row sum of |W_f| x 2^64 + largest |b_f|); r = log2(max|W_vf| / max|W_v[:, W:]|), None when
    either block is all zero. g and r are None when something is not finite."""
    return _rule(_f64(sd, "feature_linear.weight"), _f64(sd, "feature_linear.bias"), _f64(sd, "views_linears.0.weight"),
                 _f64(sd, "views_linears.0.bias"), arch["W"])


def verdict(sd, arch):
    """"eligible", "not eligible" or "undetermined" (inside the slack the equalised copy may decide either way)."""
    finite, g, r = fold_rule(sd, arch)
    if not finite or g >= GAIN_LIMIT + GAIN_SLACK or (r is not None and abs(r) >= RATIO_LIMIT + RATIO_SLACK):
        return "not eligible"
    if g <= GAIN_LIMIT - GAIN_SLACK and (r is None or abs(r) <= RATIO_LIMIT - RATIO_SLACK):
        return "eligible"
    return "undetermined"


def _row_exponents(w, b, col_exp):
    """row_exponents_kernel for one layer whose rows are scaled: w already holds every column, col_exp the producer's
    exponents per column (0 for columns that read an encoding)."""
    with np.errstate(over="ignore", invalid="ignore"):
        m1 = ((w * 2.0 ** (-col_exp)[None, :]) ** 2).sum(1) + b ** 2
    valid = (m1 > 0) & np.isfinite(m1) & (m1 < np.float64(np.finfo(np.float32).max) ** 2 * 4)
    _, e2 = np.frexp(np.where(valid, m1, 1.0))
    row_exp = (e2 + 1) >> 1                              # binade of the norm from the binade of its square
    if not valid.any():
        return np.zeros(len(b), dtype=np.int64)
    order = np.sort(row_exp[valid])
    median = order[np.searchsorted(np.arange(1, len(order) + 1), len(order) // 2 + 1)]      # first binade with > half at or below
    return np.where(valid, np.clip(median - row_exp, -30, 30), 0).astype(np.int64)


def equalised_rule(sd, arch):
    """What the device decides: (finite, g, r, folded) of the row-equalised copy (see the module's docstring)."""
    D, W, skips = arch["D"], arch["W"], arch["skips"]
    e_prev = None
    for i in range(D):
        w, b = _f64(sd, f"pts_linears.{i}.weight"), _f64(sd, f"pts_linears.{i}.bias")
        col = np.zeros(w.shape[1], dtype=np.int64)
        if i > 0:
            col[w.shape[1] - W:] = e_prev              # a skip layer reads cat[gamma(x), h]
        e_prev = _row_exponents(w, b, col)
    wf, bf = _f64(sd, "feature_linear.weight"), _f64(sd, "feature_linear.bias")
    e_f = _row_exponents(wf, bf, e_prev)
    wv, bv = _f64(sd, "views_linears.0.weight"), _f64(sd, "views_linears.0.bias")
    col = np.zeros(wv.shape[1], dtype=np.int64)
    col[:W] = e_f
    e_v = _row_exponents(wv, bv, col)
    with np.errstate(over="ignore", invalid="ignore"):
        wf_eq = wf * 2.0 ** (e_f[:, None] - e_prev[None, :])
        bf_eq = bf * 2.0 ** e_f
        wv_eq = wv * 2.0 ** (e_v[:, None] - col[None, :])
        bv_eq = bv * 2.0 ** e_v
    finite, g, r = _rule(wf_eq, bf_eq, wv_eq, bv_eq, W)
    folded = finite and g < GAIN_LIMIT and (r is None or abs(r) <= RATIO_LIMIT)
    return finite, g, r, folded


# ---- the networks ----------------------------------------------------------------------------------------------------

def _copy(sd):
    return OrderedDict((k, np.array(v, dtype=np.float32)) for k, v in sd.items())


def overflow_scaled(sd, arch, g_target):
    """The same function with W_f, b_f x2^a and W_v[:, :W] x2^-a, a the whole number that brings g to within one below
    g_target when g_target <= 124 (it must fold) and to within one above it otherwise (it must not)."""
    W = arch["W"]
    _, g0, _ = fold_rule(sd, arch)
    a = int(np.floor(g_target - g0)) if g_target <= GAIN_LIMIT - GAIN_SLACK else int(np.ceil(g_target - g0))
    out = _copy(sd)
    out["feature_linear.weight"] *= np.float32(2.0 ** a)
    out["feature_linear.bias"] *= np.float32(2.0 ** a)
    out["views_linears.0.weight"][:, :W] *= np.float32(2.0 ** -a)
    return out


def ratio_scaled(sd, arch, r_target):
    """The gamma(dir) columns x2^k, k the whole number that brings r to |r| <= |r_target| when that is 5 (folds) and to
    |r| >= |r_target| when it is 11 (does not), on r_target's side of zero."""
    W = arch["W"]
    _, _, r0 = fold_rule(sd, arch)
    inwards = abs(r_target) <= RATIO_LIMIT - RATIO_SLACK
    towards_zero = np.ceil if (r_target > 0) == inwards else np.floor      # r = r0 - k
    k = int(towards_zero(r0 - r_target))
    out = _copy(sd)
    out["views_linears.0.weight"][:, W:] *= np.float32(2.0 ** k)
    return out


def zero_block(sd, arch, which):
    out = _copy(sd)
    W = arch["W"]
    if which == "dir":
        out["views_linears.0.weight"][:, W:] = 0.0
    else:
        out["views_linears.0.weight"][:, :W] = 0.0
    return out


def base(W=256, seed=7):
    arch = arch_of(W=W)
    return _copy(synthetic.synthetic_state_dict(seed, W=W)), arch


def nonfinite_networks(W):
    """One NaN or one inf in the LAST element of each tensor the decision reads, one tensor at a time."""
    sd0, arch = base(W)
    places = {"W_f[W-1, W-1]": ("feature_linear.weight", (W - 1, W - 1)), "b_f[-1]": ("feature_linear.bias", (-1,)),
              "W_v[W/2-1, W-1]": ("views_linears.0.weight", (W // 2 - 1, W - 1)),
              "W_v[W/2-1, -1]": ("views_linears.0.weight", (W // 2 - 1, -1)), "b_v[-1]": ("views_linears.0.bias", (-1,))}
    for tag, (key, at) in places.items():
        for name, v in (("nan", np.nan), ("inf", np.inf)):
            sd = _copy(sd0)
            sd[key][at] = v
            yield f"W={W} {name} at {tag}", sd, arch, False


def boundary_networks(W):
    """(tag, state dict, arch, folds) for the decision's edges at one width."""
    sd0, arch = base(W)
    yield f"W={W} g=124", overflow_scaled(sd0, arch, 124), arch, True
    yield f"W={W} g=132", overflow_scaled(sd0, arch, 132), arch, False
    for r in (5, -5):
        yield f"W={W} r={r:+d}", ratio_scaled(sd0, arch, r), arch, True
    for r in (11, -11):
        yield f"W={W} r={r:+d}", ratio_scaled(sd0, arch, r), arch, False
    yield f"W={W} W_v[:, W:] = 0", zero_block(sd0, arch, "dir"), arch, True
    yield f"W={W} W_v[:, :W] = 0", zero_block(sd0, arch, "feature"), arch, True


def edge_networks():
    for W in (256, 100):
        yield from boundary_networks(W)
        yield from nonfinite_networks(W)


# (tag, seed, arch, multires, multires_views, i_embed): six architectures, every one asserted FOLDED
VARIANTS = (
    ("D=2", 21, arch_of(D=2, skips=()), 10, 4, 0),
    ("D=6 skips 1,3", 22, arch_of(D=6, skips=(1, 3)), 10, 4, 0),
    ("D=3 skip 0", 23, arch_of(D=3, skips=(0,)), 10, 4, 0),
    ("multires 6 / 2", 31, arch_of(input_ch=39, input_ch_views=15), 6, 2, 0),
    ("identity embedding", 32, arch_of(input_ch=3, input_ch_views=3), 10, 4, -1),
    ("W=64", 45, arch_of(W=64), 10, 4, 0),
)


def variant_state_dict(seed, arch):
    return _copy(synthetic.synthetic_state_dict(seed, D=arch["D"], W=arch["W"], skips=arch["skips"], input_ch=arch["input_ch"],
                                                input_ch_views=arch["input_ch_views"]))


def bench_pair():
    return tuple(_copy(sd) for sd in synthetic.synthetic_pair(0))


def unfoldable_twin(sd, arch=BENCH):
    """The same function, not eligible: the overflow scaling to g >= 132."""
    return overflow_scaled(sd, arch, 132)


# the live-slot sequence of test_reload_into_a_live_slot and test_deferred_refresh: other functions than the bench pair
RELOAD_SEEDS = dict(B=11, C=12, D=13)


def reload_state_dict(name):
    return _copy(synthetic.synthetic_state_dict(RELOAD_SEEDS[name]))


def hostile(case):
    """Folds whose factors are far apart in size, zero padding, and the weights a training run starts from."""
    if case == "W=128":
        return _copy(synthetic.synthetic_state_dict(41, W=128)), arch_of(W=128)
    if case == "W=100":
        return _copy(synthetic.synthetic_state_dict(44, W=100)), arch_of(W=100)
    if case == "default init":
        return _copy(synthetic.default_init_state_dict(3)), arch_of()
    sd = _copy(synthetic.synthetic_state_dict(7))
    wf, wv = sd["feature_linear.weight"], sd["views_linears.0.weight"]
    if case == "1/8 of the feature rows x2^13":        # the same function: the matching view columns x2^-13
        wf[::8] *= np.float32(2.0 ** 13)
        sd["feature_linear.bias"][::8] *= np.float32(2.0 ** 13)
        wv[:, :256:8] *= np.float32(2.0 ** -13)
    elif case == "W_f x1e3, W_v[:, :W] x1e-3":
        wf *= np.float32(1e3)
        wv[:, :256] *= np.float32(1e-3)
    elif case == "gamma(dir) columns x2^-10":
        wv[:, 256:] *= np.float32(2.0 ** -10)
    else:
        raise AssertionError(case)
    return sd, arch_of()


HOSTILE = ("1/8 of the feature rows x2^13", "W_f x1e3, W_v[:, :W] x1e-3", "gamma(dir) columns x2^-10", "W=128", "W=100",
           "default init")


def eligibility_networks():
    """The networks test_eligibility asserts as not folded: the overflow networks of
    test_nonfinite_values_born_inside_the_network and one NaN in the middle of W_f."""
    def scaled(changes):
        sd = _copy(synthetic.synthetic_state_dict(7))
        for key, f in changes.items():
            with np.errstate(over="ignore"):
                sd[key] = (sd[key] * np.float32(f)).astype(np.float32)
        return sd

    nan_w = _copy(synthetic.synthetic_state_dict(7))
    nan_w["feature_linear.weight"][17, 5] = np.nan
    return {"feature": scaled({"pts_linears.7.weight": 1e10, "feature_linear.weight": 1e30}),
            "views": scaled({"feature_linear.weight": 1e20, "views_linears.0.weight": 1e20}),
            "one NaN": nan_w}


# ---- the folded kernel's own event (mlp_kernel_h2_body.inc, the `if constexpr (fold)` block) -----------------------------------
# The event is counted where feature_linear's a-priori bound, gain x max|h| + max|b_f|, is not finite on a finite trunk
# output h. Two limits enclose it:
#   * a network the verdict calls eligible has g <= 124, a gain of at most 2^60: the bound is infinite from max|h| = 2^68 on;
#   * the kernel scales a point's activations by 2^t with t >= -60 (pick_exponent's clamp) and carries them as fp16 numbers
#     (largest 65504): a trunk output of 2^76 or more does not fit and sigma is no longer finite.
# So every point of an event test has max|h| inside [2^68, 2^76): a margin of 2^8 beyond the threshold, on every point, with
# sigma finite, does not exist (test_view_fold_cpu.py::test_event_window states this from fold_rule). event_network puts the
# points as far beyond the threshold as that window admits: the largest max|h| of the rows at 2^75, one binade below the edge.
EVENT_THRESHOLD_LOG2 = 128            # the bound is infinite from 2^128 on
EVENT_RANGE_LOG2 = 76                 # 65504 x 2^60 < 2^76: the largest activation the fp16-pair kernel represents


def event_rows(n=96):
    return np.random.RandomState(5).uniform(-1, 1, size=(n, 90)).astype(np.float32)


def trunk_max(sd, arch, x):
    """The largest |trunk output| of every embedded row, in fp64."""
    pts = np.asarray(x, dtype=np.float64)[:, :arch["input_ch"]]
    h = pts
    for i in range(arch["D"]):
        h = np.maximum(h @ _f64(sd, f"pts_linears.{i}.weight").T + _f64(sd, f"pts_linears.{i}.bias"), 0.0)
        if i in arch["skips"]:
            h = np.concatenate([pts, h], -1)
    return np.abs(h).max(1)


def event_network(arch=BENCH):
    """(state dict, log2 of the smallest distance of a row beyond the threshold). The fine bench network with
      * W_f, b_f x2^a and W_v[:, :W] x2^-a so that g lands in (123, 124] (the overflow scaling: W_vf is unchanged, eligible),
      * the trunk's last layer, weights and bias, x2^p (uniform: equalisation has nothing to move), alpha_linear x2^-p and
        rgb_linear x2^-p (the view layer is positively homogeneous in h up to its small bias and gamma(dir) terms),
    p the whole number that puts the largest max|h| of event_rows() into [2^74, 2^75)."""
    D = arch["D"]
    sd = overflow_scaled(bench_pair()[1], arch, 124)
    m = trunk_max(sd, arch, event_rows())
    p = int(np.floor(EVENT_RANGE_LOG2 - 1 - np.log2(m.max())))
    for key in (f"pts_linears.{D - 1}.weight", f"pts_linears.{D - 1}.bias"):
        sd[key] *= np.float32(2.0 ** p)
    sd["alpha_linear.weight"] *= np.float32(2.0 ** -p)
    sd["rgb_linear.weight"] *= np.float32(2.0 ** -p)
    _, g, _ = fold_rule(sd, arch)
    threshold = EVENT_THRESHOLD_LOG2 - (g - 64)          # log2 of the trunk output from which gain x m is infinite
    return sd, float(np.log2(m.min()) + p - threshold)
