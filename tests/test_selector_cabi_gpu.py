"""The selector forward through the C-ABI only (GPU box): basd_token_gram per layer -> basd_selector_frames (teacher,
with ranks) -> basd_selector_frames (student) -> basd_selector_weights -> basd_angle_weights_bwd, with no torch call
between the Gram statistics and the outputs except allocations.  Checked against the reference goldens, an fp64
restatement of d2 / t_seed, and fp64 autograd of the oracle's selector; plus the product path of BASDLoss (no library
GEMM in the selector forward, capturable in a graph).

Error bounds (rel-L2 unless stated) are about 3x the worst error measured over input seeds 0, 1, 2 of each fixture
(seed 0 only for c2_b256) on an MI355X; the measurements are recorded in DESIGN.md section 9b."""
import ctypes
import types

import pytest
import torch

from tests._golden import load, rel_l2

pytestmark = pytest.mark.gpu

STATUS_NONCONVERGED, STATUS_NONFINITE, STATUS_RANK0 = 1, 2, 4
FIXTURES = ["tiny", "tiny_rankdef", "tiny_nocls", "tiny_flat", "c1", "c2_b8", "c2_b256"]
# worst measured: d2 4.8e-7 (max abs); t_seed 4.6e-6 at D = 32, 5.5e-4 at D = 192 (c1 / c2: wider cosine spectra,
# fp32 Jacobi vectors); g_log_temp 1.5e-6, w_tok 2.9e-4 (tiny, c2_b8)
D2_BOUND = 1.5e-6        # d2 [E, L] vs the fp64 restatement on the entry's own frames (max abs)
T_SEED_BOUND = {32: 1.5e-5, 192: 1.6e-3}     # t_seed [E, L, D, D] vs the same restatement, by D
G_LT_BOUND = 5e-6        # g_log_temp vs fp64 autograd of the oracle selector
W_TOK_BOUND = 9e-4       # (s - mean) w_tok vs fp64 autograd of the oracle selector (worst extraction point)


@pytest.fixture(scope="module", autouse=True)
def _native_loaded():
    import basd_amd._native as native
    from basd_amd.losses import _ops
    assert torch.cuda.is_available()
    native.lib()
    _ops.set_ops(None)
    assert _ops.get_ops() is native


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def run_abi_selector(teacher, students, proj_s, proj_t, log_temp, g_w=None):
    """teacher: L fp32 token tensors [B, N_t, D_t], students: E fp32 [B, N_s, D_s] (device, contiguous).  Returns a
    dict of device tensors.  Between the Gram statistics and the outputs: C entries and allocations only."""
    import basd_amd._native as native
    lib = native.lib()
    dev = proj_s.device
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i64 = ctypes.c_int64
    L, E, D = len(teacher), len(students), proj_s.shape[0]
    d_s = proj_s.shape[1]
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def grams(toks, proj):
        unc = torch.zeros(len(toks), D, D, dtype=torch.float64, device=dev)
        cs = torch.zeros(len(toks), D, dtype=torch.float64, device=dev)
        for n, x in enumerate(toks):
            rows = x.shape[0] * x.shape[1]
            assert lib.basd_token_gram(_p(x), 0, i64(rows), x.shape[2], rows, i64(0), _p(proj), D, _p(unc[n]),
                                       _p(cs[n]), st) == 0
        return unc, cs, toks[0].shape[0] * toks[0].shape[1]

    def frames(unc, cs, m, with_ranks):
        n = unc.shape[0]
        out = {"ranks": torch.empty(n, dtype=torch.int32, device=dev) if with_ranks else None,
               "sigma": torch.empty(n, D, dtype=torch.float32, device=dev),
               "lam": torch.empty(n, D, dtype=torch.float64, device=dev),
               "v": torch.empty(n, D, D, dtype=torch.float32, device=dev)}
        ws = torch.empty(lib.basd_selector_frames_workspace_bytes(n, D), dtype=torch.uint8, device=dev)
        rc = lib.basd_selector_frames(_p(unc), _p(cs), n, i64(m), D, int(with_ranks), _p(out["ranks"]),
                                      _p(out["sigma"]), _p(out["lam"]), _p(out["v"]), _p(status), _p(ws),
                                      i64(ws.numel()), st)
        assert rc == 0, lib.basd_last_error()
        return out

    t_unc, t_cs, m_t = grams(teacher, proj_t)
    s_unc, s_cs, m_s = grams(students, proj_s)
    tf = frames(t_unc, t_cs, m_t, True)
    sf = frames(s_unc, s_cs, m_s, False)
    res = {"ranks": tf["ranks"], "vm_t": tf["v"], "sw": tf["sigma"], "v_s": sf["v"], "lam_s": sf["lam"],
           "status": status}
    for k in ("weights", "pre", "d2"):
        res[k] = torch.empty(E, L, dtype=torch.float32, device=dev)
    res["t_seed"] = torch.empty(E, L, D, D, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.basd_selector_weights_workspace_bytes(E, L, D), dtype=torch.uint8, device=dev)
    rc = lib.basd_selector_weights(_p(sf["v"]), _p(tf["ranks"]), _p(tf["v"]), _p(tf["sigma"]), _p(log_temp), E, L, D,
                                   _p(res["weights"]), _p(res["pre"]), _p(res["d2"]), _p(res["t_seed"]), _p(status),
                                   _p(ws), i64(ws.numel()), st)
    assert rc == 0, lib.basd_last_error()
    if g_w is not None:
        res["g_log_temp"] = torch.empty(E, dtype=torch.float32, device=dev)
        res["w_tok"] = torch.empty(E, d_s, d_s, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.basd_angle_weights_bwd_workspace_bytes(E, D, d_s), dtype=torch.uint8, device=dev)
        rc = lib.basd_angle_weights_bwd(_p(g_w), None, _p(res["weights"]), _p(res["d2"]), _p(log_temp),
                                        _p(res["t_seed"]), _p(sf["v"]), _p(sf["lam"]), _p(proj_s), E, L, D, d_s,
                                        _p(res["g_log_temp"]), _p(res["w_tok"]), _p(ws), i64(ws.numel()), st)
        assert rc == 0, lib.basd_last_error()
    torch.cuda.synchronize()
    return res


def restate_fp64(v_s, vm_t, sw, ranks):
    """d2 [E, L] and t_seed [E, L, D, D] in fp64 from the entry's own frames: A = V_s V_t^T, A_bar = rows b < k_j,
    cosines / left vectors from an fp64 SVD of A_bar, Phi = U diag(gsig / sigma) U^T, T = A A_bar^T Phi (rows >= k_j)."""
    v_s, vm_t, sw = v_s.double().cpu(), vm_t.double().cpu(), sw.double().cpu()
    ranks = ranks.cpu().tolist()
    E, D = v_s.shape[0], v_s.shape[1]
    L = vm_t.shape[0]
    eps = float(torch.finfo(torch.float32).eps)
    d2 = torch.zeros(E, L, dtype=torch.float64)
    t_seed = torch.zeros(E, L, D, D, dtype=torch.float64)
    for j in range(L):
        k = ranks[j]
        den = sw[j].sum()
        for i in range(E):
            a = v_s[i] @ vm_t[j].T
            ab = a.clone()
            ab[k:] = 0
            u, s, _ = torch.linalg.svd(ab)
            sc = s.clamp(max=1.0 - eps)
            th = torch.acos(sc)
            d2[i, j] = (sw[j] * th * th).sum() / den
            ok = (s <= 1.0 - eps) & (s > 1e-9)
            gs = torch.where(ok, sw[j] * 2.0 * th * (-1.0 / torch.sqrt(1.0 - sc * sc)) / den, torch.zeros_like(s))
            phi = (u * (gs / s.clamp_min(1e-300))) @ u.T
            t = a @ ab.T @ phi
            t[:k] = 0
            t_seed[i, j] = t
    return d2, t_seed


def oracle_selector_grads(teacher, students, proj_s, proj_t, log_temp, ranks, g_w):
    """fp64 autograd of the reference selector (oracle pca_frame / grassmann_distance, softmax of -d2 / softplus):
    d <g_w, weights> / d log_temp and / d student tokens."""
    from oracle import basd_oracle as O
    ps, pt = proj_s.double().cpu(), proj_t.double().cpu()
    bases, sws = [], []
    for x, k in zip(teacher, ranks):
        s, vt = O.pca_frame(x.double().cpu().reshape(-1, x.shape[-1]) @ pt.T)
        bases.append(vt[:k].T.contiguous())
        sws.append(s[:k])
    s64 = [s.double().cpu().requires_grad_(True) for s in students]
    lt = log_temp.double().cpu().requires_grad_(True)
    tau = torch.nn.functional.softplus(lt)
    total = 0.0
    for i, s in enumerate(s64):
        _, vt_s = O.pca_frame(s.reshape(-1, s.shape[-1]) @ ps.T)
        d2 = torch.stack([O.grassmann_distance(vt_s, bases[j], sws[j]) for j in range(len(bases))])
        w = torch.softmax(-d2 / tau[i], dim=0)
        total = total + (g_w[i].double().cpu() * w).sum()
    total.backward()
    return lt.grad, [s.grad for s in s64]


def _case(name):
    shape, inputs, gold = load(name)
    dev = torch.device("cuda")
    layers = inputs["token_layers"]
    teacher = [inputs["teacher_tokens"][j].float().contiguous().to(dev) for j in range(shape.L_t)]
    students = [inputs["student_tokens"][l].float().contiguous().to(dev) for l in layers]
    return shape, gold, teacher, students, gold["proj_s"].float().to(dev), gold["proj_t"].float().to(dev), \
        gold["log_temperatures"].float().to(dev)


def selector_errors(teacher, students, proj_s, proj_t, log_temp, with_grads, seed=0):
    """-> (result dict, {error name: value}) of one C-ABI selector run (also used to set the bounds above)."""
    E, L = len(students), len(teacher)
    g_w = torch.randn(E, L, generator=torch.Generator().manual_seed(100 + seed)).float().cuda() if with_grads else None
    res = run_abi_selector(teacher, students, proj_s, proj_t, log_temp, g_w)
    d2, t_seed = restate_fp64(res["v_s"], res["vm_t"], res["sw"], res["ranks"])
    err = {"d2": float((res["d2"].cpu().double() - d2).abs().max()), "t_seed": rel_l2(res["t_seed"].cpu(), t_seed)}
    if with_grads:
        g_lt, g_s = oracle_selector_grads(teacher, students, proj_s, proj_t, log_temp, res["ranks"].tolist(), g_w)
        err["g_log_temp"] = rel_l2(res["g_log_temp"].cpu(), g_lt)
        worst = 0.0
        for i, s in enumerate(students):
            sf = s.double().cpu().reshape(-1, s.shape[-1])
            got = (sf - sf.mean(dim=0, keepdim=True)) @ res["w_tok"][i].double().cpu()
            worst = max(worst, rel_l2(got, g_s[i].reshape(got.shape)))
        err["w_tok"] = worst
    return res, err


@pytest.mark.parametrize("name", FIXTURES)
def test_selector_cabi_matches_goldens(name):
    shape, gold, teacher, students, proj_s, proj_t, log_temp = _case(name)
    with_grads = name in ("tiny", "c2_b8")            # fp64 spectra without repeated singular values
    res, err = selector_errors(teacher, students, proj_s, proj_t, log_temp, with_grads)
    print(f"{name}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert int(res["status"].item()) == 0
    for kind in ("hard", "soft"):
        if f"{kind}/ranks" not in gold:
            continue
        assert res["ranks"].cpu().tolist() == gold[f"{kind}/ranks"].tolist()
        torch.testing.assert_close(res["weights"].cpu(), gold[f"{kind}/weights"], atol=2e-6, rtol=0)
        torch.testing.assert_close(res["pre"].cpu(), gold[f"{kind}/pre_softmax"], atol=2e-5, rtol=1e-4)
    assert err["d2"] < D2_BOUND, err
    assert err["t_seed"] < T_SEED_BOUND[shape.D_s], err
    if with_grads:
        assert err["g_log_temp"] < G_LT_BOUND, err
        assert err["w_tok"] < W_TOK_BOUND, err


def test_nonfinite_token_sets_the_status_bit():
    shape, gold, teacher, students, proj_s, proj_t, log_temp = _case("tiny")
    teacher[1] = teacher[1].clone()
    teacher[1][0, 3, 5] = float("nan")
    res = run_abi_selector(teacher, students, proj_s, proj_t, log_temp)        # every entry returned 0
    assert int(res["status"].item()) & STATUS_NONFINITE


def test_rank0_teacher_layer_sets_the_status_bit():
    shape, gold, teacher, students, proj_s, proj_t, log_temp = _case("tiny")
    teacher[2] = torch.zeros_like(teacher[2])
    res = run_abi_selector(teacher, students, proj_s, proj_t, log_temp)
    assert int(res["status"].item()) & STATUS_RANK0
    assert res["ranks"].cpu().tolist()[2] == 0


# --------------------------------------------------------------------------------------------------------------------
# product path: BASDLoss routes the selector forward through the entries
def _c2_loss():
    from basd_amd.losses import BASDLoss
    shape, inputs, gold = load("c2_b8")
    dev = torch.device("cuda")
    mod = BASDLoss(torch.nn.CrossEntropyLoss(label_smoothing=1.0 / shape.C), shape.D_s, shape.D_t, shape.L_s,
                   shape.N_s, config=types.SimpleNamespace(num_extraction_points=shape.E),
                   teacher_has_cls_token=shape.has_cls)
    with torch.no_grad():
        mod.layer_selector.proj_s.copy_(gold["proj_s"])
        mod.layer_selector.proj_t.copy_(gold["proj_t"])
        mod.layer_selector.log_temperatures.copy_(gold["log_temperatures"])
    mod = mod.to(dev)
    s_tok = {l: t.to(dev).requires_grad_(True) for l, t in inputs["student_tokens"].items()}
    t_tok = {j: t.to(dev) for j, t in inputs["teacher_tokens"].items()}
    t_att = {j: t.to(dev) for j, t in inputs["teacher_attns"].items()}
    return shape, gold, mod, inputs["logits"].to(dev), inputs["targets_hard"].to(dev), s_tok, t_tok, t_att


def test_selector_forward_runs_no_library_gemm():
    from basd_amd.losses._ops import record_library_gemms
    shape, gold, mod, logits, targets, s_tok, t_tok, t_att = _c2_loss()
    with torch.no_grad(), record_library_gemms() as seen:
        mod.layer_selector.mixing_weights(s_tok, t_tok, mod.token_layers)
    torch.cuda.synchronize()
    assert not ({"aten::bmm", "aten::mm", "aten::matmul", "aten::einsum"} & seen), seen
    torch.testing.assert_close(mod.layer_selector.last_weights.cpu(), gold["hard/weights"], atol=2e-6, rtol=0)


def test_captured_loss_matches_eager():
    shape, gold, mod, logits, targets, s_tok, t_tok, t_att = _c2_loss()
    logits.requires_grad_(True)
    leaves = list(s_tok.values()) + [logits, mod.layer_selector.log_temperatures]

    def step():
        for t in leaves:
            t.grad = None
        loss = mod(logits, targets, s_tok, t_tok, t_att)
        loss.backward()
        return loss

    loss_e = step().detach().clone()
    want = [t.grad.detach().clone() for t in leaves]
    w_e = mod.layer_selector.last_weights.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaves:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g = step()
    graph.replay()
    torch.cuda.synchronize()
    torch.testing.assert_close(loss_g.detach(), loss_e, rtol=1e-5, atol=0)
    torch.testing.assert_close(mod.layer_selector.last_weights, w_e, atol=1e-6, rtol=0)
    for t, g in zip(leaves, want):
        assert rel_l2(t.grad, g) < 1e-4
