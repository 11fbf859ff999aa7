"""
The update half of a training iteration on the GPU against the independent float64 statement (tests/adam_reference.py):
optimizer.adam_update (dense and from view payloads), dist.sh_gradients_from_views, and the hand-off
backward() -> grads_from_backward -> adam_update, on the case matrix of tests/test_adam_reference.py.

Criterion, as in test_gpu_f64_reference.py: per array, the kernel's error against float64 may be at most 3 x the oracle's
error on the same inputs plus a floor of one float32 rounding of the compared quantity -- 2^-23 of max|x| for a moment,
2^-23 max|p| / lr for a parameter (errors of parameters are in units of one full step, lr).  Kernel and oracle share the
float32 expression tree with correctly rounded division and square root and the same host powf; they may differ by FMA
contraction only.  The oracle's errors are those of this run, not the recorded ones.
"""
import numpy as np
import pytest

from conftest import pkg, sub
import adam_reference as A
import dssim_reference as DS
import f64_reference as F
import parity
import test_adam_reference as T
import test_f64_reference as R

pytestmark = pytest.mark.gpu
GROUPS = A.GROUPS
ROUND = 2.0 ** -23


def _dev(d):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _host(d):
    return {k: v.detach().cpu().numpy().copy() for k, v in d.items()}


def figures(got, ref64, lrs):
    """{array: the issue's error figure} of a float32 (P, M, V) against the statement's."""
    out = {}
    for i, pre in enumerate(("", "m_", "v_")):
        for k in GROUPS:
            x, x64 = np.asarray(got[i][k], np.float64).reshape(ref64[i][k].shape), ref64[i][k]
            if i == 0:
                out[k] = float(np.abs(x - x64).max() / A._f(lrs[k])) if np.isfinite(x).all() else float("inf")
            else:
                out[pre + k] = T._rel(x, x64)
    return out


def floors(ref64, lrs):
    return {**{k: ROUND * float(np.abs(ref64[0][k]).max()) / A._f(lrs[k]) for k in GROUPS},
            **{pre + k: ROUND for pre in ("m_", "v_") for k in GROUPS}}


def check(label, kernel, yardstick, ref64, lrs, arrays=None):
    """Assert the criterion for `arrays` (default all fifteen) and return the printed rows."""
    e_k, e_o, fl = figures(kernel, ref64, lrs), figures(yardstick, ref64, lrs), floors(ref64, lrs)
    rows = [(name, e_o[name], e_k[name]) for name in (arrays or list(e_k))]
    print(f"\n{label}\n  array          oracle vs f64   kernel vs f64   floor")
    for name, o, k in rows:
        print("  %-14s %.3e       %.3e       %.3e" % (name, o, k, fl[name]))
    for name, o, k in rows:
        assert k <= 3.0 * o + fl[name], f"{label}: {name}: kernel {k:.3e} vs float64; oracle {o:.3e}, floor {fl[name]:.3e}"
    return rows


def _payloads(spec, positions, V=2):
    """Two view payloads for a case's sh_views= run (all zero where the case's gradients are)."""
    n = positions.shape[0]
    rng = np.random.default_rng(spec["seed"] + 500)
    pay = np.zeros((V, 3 * n + 4), np.float32)
    if spec["grads"] != "zero":
        pay[:, :3 * n] = (rng.normal(0, 1e-3, (V, 3 * n)) * (rng.uniform(0, 1, (V, 3 * n)) > 0.3)).astype(np.float32)
    cams = rng.normal(0, 3, (V, 3)).astype(np.float32)
    cams[0] = positions[0]                                       # Gaussian 0 at view 0's camera centre
    pay[:, 3 * n:3 * n + 3] = cams
    return pay


def _kernel_step(P, G, M, V, hyper, lrs, **views):
    gsr = pkg()
    dP, dM, dV = _dev(P), _dev(M), _dev(V)
    dG = {k: (None if G[k] is None else _dev({k: G[k]})[k]) for k in GROUPS}
    gsr.optimizer.adam_update(dP, dG, dM, dV, lrs, **hyper, **views)
    return _host(dP), _host(dM), _host(dV)


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_adam_kernels_against_f64(oracle, name):
    import torch
    gsr = pkg()
    c = T.oracle_case(oracle, name)
    P, G, M, V, hyper = c["inputs"]
    # dense path: the oracle's run and the statement are the CPU test's
    got = _kernel_step(P, G, M, V, hyper, T.LRS)
    rows = check(f"{name} (dense)", got, c["got"], c["ref64"], T.LRS)
    for x in got:
        assert all(np.isfinite(x[k]).all() for k in GROUPS)
    # sh_views= path: the SH gradient the kernel forms from two payloads is the one dist.sh_gradients_from_views rebuilds (bit for
    # bit: test_adam_from_view_payloads_is_the_same_step), so the statement and the oracle are fed that rebuilt gradient
    pay = _payloads(dict(T.CASES)[name], P["positions"])
    d_pay = torch.as_tensor(pay).cuda()
    g_sh = gsr.dist.sh_gradients_from_views(torch.as_tensor(P["positions"]).cuda(), d_pay, 3, average=True).cpu().numpy()
    Gv = dict(G, shs=g_sh)
    inputs = (P, Gv, M, V, hyper)
    ref64 = A.adam_step(P, Gv, M, V, T.LRS, **hyper)
    got_v = _kernel_step(P, dict(G, shs=None), M, V, hyper, T.LRS, sh_views=d_pay, sh_degree=3)
    rows_v = check(f"{name} (sh_views)", got_v, T.run_oracle(oracle, inputs), ref64, T.LRS)
    T.record_margins("kernel_vs_f64", {name: [(a, k, o) for a, o, k in rows], name + "/sh_views": [(a, k, o) for a, o, k in rows_v]})


def test_adam_trajectory_against_f64(oracle):
    """200 consecutive steps from zero moments, 70 % of each step's gradients exactly zero; compared after 1, 10 and 200."""
    o_states = {n: s32 for n, s32, _, _ in T.trajectory(lambda P, G, M, V, h: T.run_oracle(oracle, (P, G, M, V, h)))}
    gsr = pkg()
    state = {}

    def step(P, G, M, V, hyper):
        if not state:
            state.update(P=_dev(P), M=_dev(M), V=_dev(V))
        gsr.optimizer.adam_update(state["P"], _dev(G), state["M"], state["V"], T.LRS, **hyper)
        return None, None, None

    table = {}
    for n_steps, _, s64, _ in T.trajectory(step):
        got = (_host(state["P"]), _host(state["M"]), _host(state["V"]))
        rows = check(f"trajectory after {n_steps} steps", got, o_states[n_steps], s64, T.LRS)
        table[f"trajectory_step{n_steps}"] = [(a, k, o) for a, o, k in rows]
    T.record_margins("kernel_vs_f64", table)


# float32 model of the rebuilt gradient, per Gaussian and channel: direction (a difference, three squares and two sums, a root, a
# division: <= 5 roundings per component), a basis polynomial of degree <= 3 in it (3 x 5 for the components, <= 5 for its own
# operations) whose monomials sum to at most 2 in magnitude -> 40 u sum_v |dL_drgb_v|; V products and V sums, the scale, and one more
# sum per extra chunk -> (V + 2) u of the same.
def _sh_bound(pay, n, V, scale):
    return (40 + V + 2) * T.U * abs(A._f(scale)) * np.abs(pay[:, :3 * n].astype(np.float64)).reshape(V, n, 1, 3).sum(0)


@pytest.mark.parametrize("name", T.SH_NAMES)
def test_sh_view_rebuild_against_f64(name):
    import torch
    gsr = pkg()
    means, pay, degree, scale, at = T.build_sh_case(name)
    n, V = means.shape[0], pay.shape[0]
    d_means, d_pay = torch.as_tensor(means).cuda(), torch.as_tensor(pay).cuda()
    nb = (degree + 1) ** 2
    worst = {}
    for label, kw, s in (("average", dict(average=True), 1.0 / V), ("sum", dict(average=False), 1.0), ("scale", dict(scale=scale), scale)):
        got = gsr.dist.sh_gradients_from_views(d_means, d_pay, degree, **kw).cpu().numpy().reshape(n, 16, 3)
        ref = A.sh_gradient_from_views(means, pay, degree, s).reshape(n, 16, 3)
        bound = np.broadcast_to(_sh_bound(pay, n, V, s), ref.shape)
        err = np.abs(got - ref)
        assert (err <= bound).all(), f"{name} {label}: {float((err / np.maximum(bound, 1e-300)).max()):.2f} x the float32 model"
        worst[label] = float((err / np.maximum(bound, 1e-300)).max())
        assert not got[:, nb:].any(), f"{name} {label}: gradient above degree {degree}"
        assert np.abs(ref).max() > 0 or n == 1
        if at is not None:                                      # view 0 must contribute exactly nothing to the Gaussian at its camera
            pay0 = pay.copy()
            pay0[0, 3 * at:3 * at + 3] = 0.0
            again = gsr.dist.sh_gradients_from_views(d_means, torch.as_tensor(pay0).cuda(), degree, **kw).cpu().numpy().reshape(n, 16, 3)
            assert np.array_equal(again[at], got[at]), f"{name} {label}: the view at the camera centre contributed"
            if V == 1:
                assert not got[at].any()
    print(f"\n{name}: rebuilt SH gradient, worst error / float32 model: {worst}")
    if V > T.MAX_VIEWS:                                             # adam_update takes at most GSR_MAX_VIEWS payloads
        return
    # the fused update against the statement's step fed the statement's own SH gradient; yardstick: the library's dense path on
    # the rebuilt gradient
    P, G, M, Vm, hyper = T.build_case(dict(n=n, it=3, seed=77 + n, grads="dense", moments="real"))
    P["positions"] = means
    g64 = A.sh_gradient_from_views(means, pay, degree, scale)
    ref64 = A.adam_step(P, dict(G, shs=g64), M, Vm, T.LRS, **hyper)
    fused = _kernel_step(P, dict(G, shs=None), M, Vm, hyper, T.LRS, sh_views=d_pay, sh_degree=degree, sh_scale=scale)
    rebuilt = gsr.dist.sh_gradients_from_views(d_means, d_pay, degree, scale=scale).cpu().numpy()
    dense = _kernel_step(P, dict(G, shs=rebuilt), M, Vm, hyper, T.LRS)
    check(f"{name} (fused update, scale {scale:.3g})", fused, dense, ref64, T.LRS)
    # and absolutely: the first moment of the SH group carries the rebuilt gradient's error, (1 - beta1) of it, plus its own roundings
    dm = np.abs(fused[1]["shs"].reshape(n, 16, 3) - ref64[1]["shs"].reshape(n, 16, 3))
    lim = 0.1 * np.broadcast_to(_sh_bound(pay, n, V, scale), dm.shape) + 4 * T.U * np.abs(ref64[1]["shs"]).max()
    assert (dm <= lim).all(), f"{name}: m_shs {float((dm / lim).max()):.2f} x the float32 model"


# ---------------------------------------------------------------------------------------------------------------- the hand-off
HAND_CASE = "64x48_n65"                                              # N % 4 = 1, degree 3, every gradient group alive
HAND_LRS = {"positions": 3.0e-2, "scales": 2.0e-3, "rotations": 7.0e-3, "opacities": 1.1e-2, "shs": 1.7e-2}
LAMBDA = 0.2


def _scene_of(P, n):
    return {"means": P["positions"], "scales": P["scales"], "rotations": P["rotations"], "opacities": P["opacities"].reshape(n, 1),
            "shs": P["shs"].reshape(n, 16, 3)}


def _second_view(cameras, c):
    """Another camera on the same scene: the case's camera turned by 0.15 rad about its y axis and moved sideways."""
    kw, cam = c["kw"], c["cam"]
    Rw = np.asarray(kw["viewmatrix"], np.float64)[:3, :3].T            # rows: camera axes (train.py convention: view = [R^T 0; t 1])
    a = 0.15
    turn = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    centre = np.asarray(cam["camera_center"], np.float64)[:3] + 0.5 * Rw[0]
    cam2 = R.camera(cameras, turn @ Rw, centre, kw["image_width"], kw["image_height"])
    kw2 = dict(kw, viewmatrix=cam2["world_to_camera"], projmatrix=cam2["full_proj_matrix"], tan_fovx=cam2["tan_fovx"],
               tan_fovy=cam2["tan_fovy"], campos=cam2["camera_center"])
    return kw2


def _f64_view(oracle, P_host, n, kw, target, gpu_buf):
    """The float64 chain of one view at the kernel's current parameters: forward image, D-SSIM pixel gradient, backward."""
    import torch
    sc = _scene_of(P_host, n)
    kws = dict(kw, means3D=sc["means"], opacity=sc["opacities"], scales=sc["scales"], rotations=sc["rotations"], sh=sc["shs"])
    buf = oracle.render_gaussians(**kws)[2]                           # the list order, from the float32 restatement
    for k in ("point_list", "ranges"):
        parity.assert_exact(k, gpu_buf[k], buf[k])
    pre = F.preprocess_f64(sc, kws, int(kw["degree"]), float(kw["scale_modifier"]))
    with torch.no_grad():
        img = F.blend_f64(pre["xy"], pre["conic"], pre["opacity"], pre["colour"], pre["depth"], buf["point_list"], buf["ranges"],
                          pre["cam"].bg, pre["cam"].W, pre["cam"].H)[0]
    y = torch.as_tensor(np.asarray(target, np.float64))
    assert float((img - y).abs().min()) >= 1e-3, "an L1 sign sits near a tie"
    dpix = DS.pixel_grad(img, y, LAMBDA, "gaussian").numpy()
    g = F.backward_f64(sc, kws, buf["point_list"], buf["ranges"], dpix, pre=pre)
    return {"positions": g["dL_dmean3D"], "scales": g["dL_dscale"], "rotations": g["dL_drot"],
            "opacities": g["dL_dopacity"].reshape(n), "shs": g["dL_dshs"]}


def _gpu_view(gsr, P, kw, target, mode):
    fkw = dict(kw, means3D=P["positions"], opacity=P["opacities"], scales=P["scales"], rotations=P["rotations"], sh=P["shs"])
    img, _, buf = gsr.render_gaussians(**fkw)
    _, _, dpix = gsr.loss.l1_dssim_loss_and_gradients(img, target, LAMBDA)
    g = gsr.backward(background=kw["background"], means3D=P["positions"], dL_dpixels=dpix, opacity=P["opacities"], shs=P["shs"],
                     scales=P["scales"], rotations=P["rotations"], scale_modifier=kw["scale_modifier"], viewmatrix=kw["viewmatrix"],
                     projmatrix=kw["projmatrix"], tan_fovx=kw["tan_fovx"], tan_fovy=kw["tan_fovy"], image_height=kw["image_height"],
                     image_width=kw["image_width"], campos=kw["campos"], radii=buf["radii"], means2D=buf["points_xy_image"],
                     conic_opacity=buf["conic_opacity"], rgb=buf["colors"], cov3Ds=buf["cov3Ds"], clamped=buf["clamped_state"],
                     binning_buffer={"point_list": buf["point_list"]},
                     img_buffer={"ranges": buf["ranges"], "final_Ts": buf["final_Ts"], "n_contrib": buf["n_contrib"]},
                     degree=kw["degree"], sh_gradient=mode)
    return img, buf, g


@pytest.mark.parametrize("mode", ["dense", "factored"])
def test_one_training_step_hands_the_right_arrays_over(oracle, cameras, mode):
    """render -> loss (lambda_dssim 0.2) -> backward -> grads_from_backward -> adam_update, two iterations, as examples/train.py
    makes the calls: one view with the dense SH gradient, or two views with factored payloads into sh_views and averaged small
    arenas.  First half: the moments must be those of the float64 chain's gradients (a wrong array, offset or scale shows
    there).  Second half: the parameters against the statement fed the kernel's own gradients (the update alone)."""
    import torch
    gsr = pkg()
    c = R.oracle_case(oracle, cameras, HAND_CASE)
    sc, n = c["sc"], c["sc"]["means"].shape[0]
    assert n % 4 != 0
    kws = [dict(c["kw"])] + ([_second_view(cameras, c)] if mode == "factored" else [])
    nv = len(kws)
    P = _dev({"positions": sc["means"], "scales": sc["scales"], "rotations": sc["rotations"], "opacities": sc["opacities"].reshape(-1),
              "shs": sc["shs"].reshape(-1, 3)})
    M, V = gsr.optimizer.make_state(P)
    rng = np.random.default_rng(4)
    targets = []
    for kw in kws:                                                    # every pixel 2 .. 3 away from the first render: no step of these two brings an L1 sign near a tie
        img0 = _gpu_view(gsr, P, kw, torch.zeros(kw["image_height"], kw["image_width"], 3).cuda(), "dense")[0].cpu().numpy()
        targets.append((img0 + rng.choice([-1.0, 1.0], img0.shape) * rng.uniform(2.0, 3.0, img0.shape)).astype(np.float32))
    d_targets = [torch.as_tensor(t).cuda() for t in targets]
    b1, b2 = A._f(0.9), A._f(0.999)
    M64 = {k: np.zeros(tuple(P[k].shape)) for k in GROUPS}
    caught_stale_directions = False
    for it in range(2):
        before = (_host(P), _host(M), _host(V))
        arena, payloads, g64 = None, [], None
        for kw, tgt, d_tgt in zip(kws, targets, d_targets):
            _, buf, g = _gpu_view(gsr, P, kw, d_tgt, mode)
            arena = g["_arena"] if arena is None else arena.add_(g["_arena"])
            payloads.append(g["_view_payload"])
            gv = _f64_view(oracle, before[0], n, kw, tgt, {k: parity.to_np(buf[k]) for k in ("point_list", "ranges")})
            g64 = gv if g64 is None else {k: g64[k] + gv[k] for k in GROUPS}
        g64 = {k: x / nv for k, x in g64.items()}
        hyper = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, iteration=it)
        if mode == "factored":
            arena.mul_(1.0 / nv)
            grads = gsr.dist.small_arena_views(arena, n)
            grads["dL_dshs"] = None
            pay_host = np.stack([p.cpu().numpy() for p in payloads])
            # the kernel's own SH gradient: what it forms from the payloads inside the update is, bit for bit, this rebuild
            # (test_adam_from_view_payloads_is_the_same_step), taken here with the positions of BEFORE the step
            rebuilt = gsr.dist.sh_gradients_from_views(P["positions"], torch.stack(payloads), 3, scale=1.0 / nv).cpu().numpy()
            gsr.optimizer.adam_update(P, gsr.optimizer.grads_from_backward(grads), M, V, HAND_LRS, **hyper, sh_views=payloads,
                                      sh_degree=3, sh_scale=1.0 / nv)
            own = {k: grads["dL_d" + s].cpu().numpy() for k, s in (("positions", "mean3D"), ("scales", "scale"), ("rotations", "rot"), ("opacities", "opacity"))}
            own["shs"] = rebuilt
        else:
            grads = gsr.dist.arena_views(arena, n)
            gk = gsr.optimizer.grads_from_backward(grads)
            own = _host(gk)
            gsr.optimizer.adam_update(P, gk, M, V, HAND_LRS, **hyper)
        after = (_host(P), _host(M), _host(V))
        # first half: m / (1 - beta1) is the float64 chain's gradient at iteration 0, and its own first moment over (1 - beta1) after
        M64 = {k: b1 * M64[k] + (1 - b1) * g64[k].reshape(M64[k].shape) for k in GROUPS}
        for k in GROUPS:
            parity.assert_grad(f"it {it} m_{k} / (1 - beta1)", after[1][k] / (1 - b1), M64[k] / (1 - b1))
            if it == 0:
                parity.assert_grad(f"sqrt(v_{k} / (1 - beta2))", np.sqrt(after[2][k] / (1 - b2)), np.abs(g64[k]).reshape(after[2][k].shape))
        # second half: the update alone
        G32 = {k: np.asarray(own[k], np.float32).reshape(before[0][k].shape) for k in GROUPS}
        inputs = (before[0], G32, before[1], before[2], hyper)
        ref64 = A.adam_step(*inputs[:4], HAND_LRS, **hyper)
        yard = T.run_oracle(oracle, inputs, HAND_LRS)
        check(f"hand-off {mode}, iteration {it}", after, yard, ref64, HAND_LRS, arrays=list(GROUPS))
        if mode == "factored":
            # Which positions gave the SH directions shows in the first moment of the SH group, m' = b1 m + (1 - b1) g: it must
            # be the statement's own gradient at the positions BEFORE the step, within the rebuild's float32 model (_sh_bound)
            # and the moment's own roundings, element by element; the statement at the positions AFTER the step must not fit.
            # (The parameters are not judged against the statement's own gradient: where two views' contributions cancel
            # to |g| < epsilon the step is g / (|g| + epsilon), and the rebuild's float32 rounding of 1e-12 is worth 1e-4 of a
            # step -- measured 8.7e-5 -- which is float32's resolution of the gradient, not the update.  They are compared below.)
            m0 = before[1]["shs"].astype(np.float64)
            lim = ((1 - b1) * np.broadcast_to(_sh_bound(pay_host, n, nv, 1.0 / nv), (n, 16, 3)).reshape(n * 16, 3)
                   + 4 * T.U * (b1 * np.abs(m0) + (1 - b1) * np.abs(rebuilt)))
            fits = {}
            for when, pos in (("before", before[0]["positions"]), ("after", ref64[0]["positions"])):
                g_own = A.sh_gradient_from_views(pos, pay_host, 3, 1.0 / nv)
                ref_w = A.adam_step(before[0], dict(G32, shs=g_own), before[1], before[2], HAND_LRS, **hyper)
                fits[when] = (float((np.abs(after[1]["shs"] - ref_w[1]["shs"]) / np.maximum(lim, 1e-300)).max()),
                              figures(after, ref_w, HAND_LRS)["shs"])
            print(f"  SH directions: m_shs error / model, parameter error in steps: {fits}")
            assert fits["before"][0] <= 1.0, f"m_shs is not the gradient at the pre-step directions: {fits}"
            assert fits["after"][0] > 1.0, f"SH updated with post-step directions would have passed: {fits}"
            caught_stale_directions |= fits["after"][1] > 3.0 * fits["before"][1] + floors(ref64, HAND_LRS)["shs"]
    assert caught_stale_directions or mode == "dense", "SH parameters updated with post-step directions would have passed"
