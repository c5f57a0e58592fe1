"""CPU: the one-product-logit bound (catalog.ondemand_widening(products=1); DESIGN.md (d), "One
product per logit term") holds in a numpy emulation of the kernel's arithmetic.

The emulation follows catalog_score_x3b_kernel<..., ONE = true>: power-of-two scales as pow2_scale
(S_A from Wmax and the 32-row chunk's largest |h|, S_t from the candidate row's largest |t|),
A = fl32(fl32(W1 S_A) h) and B = t S_t rounded to f16, exact products, fp32 accumulation from
fl32(S b1) in the kernel's K order, then fl32 sum of fl32(w2 / S) ReLU(acc). It is compared with
float64 logits for EVERY (item, candidate) pair of small models:

  |a1 - a64| <= eta_a     (eta_a re-stated here from the derivation, not read from the code)
  e64 in [e1 (1 - eta'), e1 (1 + eta')]

(the float64 logit stands in for the fp16x6 kernel's, whose own error terms the bound also holds),
and eta' of ondemand_widening must be the eta_a (1 + eta_a) + 2^-20 of that statement. products=3
must return what the function returned before the argument existed, bit for bit.
"""
import numpy as np
import pytest
import torch

F = np.float32


def pow2_scale(m):
    m = F(m)
    if not (m > 0) or not np.isfinite(m):
        return F(1)
    bits = int(np.array(m, F).view(np.uint32))
    ex = ((bits >> 23) & 255) - 127
    if ((bits >> 23) & 255) == 0:
        ex = -127
    e = min(120, max(-120, 13 - ex))
    return F(2.0) ** F(e)


def _pad(x, rows, cols):
    out = np.zeros((rows, cols), F)
    out[:x.shape[0], :x.shape[1]] = x
    return out


def emulate_one_product_logits(eh, et, W1, b1, w2):
    """a1 [J, C] float32 as the one-product kernel forms it (see the module docstring)."""
    J, D = eh.shape
    C = et.shape[0]
    H = W1.shape[0]
    DP = 32 if D <= 32 else 64
    HP = 32 if H <= 32 else 64
    DH = DP // 2
    eh, et, W1 = _pad(eh, J, DP), _pad(et, C, DP), _pad(W1, HP, DP)
    b1 = np.concatenate([b1, np.zeros(HP - H, F)]).astype(F)
    w2 = np.concatenate([w2.reshape(-1), np.zeros(HP - H, F)]).astype(F)
    Wmax = np.abs(W1).max()
    St = np.array([pow2_scale(np.abs(et[c]).max()) for c in range(C)], F)          # [C]
    Bh = (et * St[:, None]).astype(F).astype(np.float16).astype(np.float64)         # [C, DP]
    korder = [hh * DH + 8 * s + x for s in range(DH // 8) for hh in (0, 1) for x in range(8)]
    a = np.empty((J, C), F)
    for j0 in range(0, J, 32):
        h = eh[j0:j0 + 32]
        SA = pow2_scale(F(Wmax) * np.abs(h).max())
        wv = (W1 * SA).astype(F)
        A = (wv[None, :, :] * h[:, None, :]).astype(F)                              # [j, HP, DP], fl32
        Ah = A.astype(np.float16).astype(np.float64)
        S = (SA * St).astype(F)                                                     # [C]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            invS = (F(1) / S).astype(F)
            acc = np.broadcast_to((b1[None, :] * S[:, None]).astype(F)[None], (len(h), C, HP)).copy()
            for k in korder:
                prod = Ah[:, None, :, k] * Bh[None, :, k, None]                     # exact in float64
                acc = (acc.astype(np.float64) + prod).astype(F)
            ws = (w2[None, :] * invS[:, None]).astype(F)                            # [C, HP]
            ap = np.zeros((len(h), C), F)
            for i in range(HP):
                ap = (ap + (ws[None, :, i] * np.maximum(acc[:, :, i], F(0))).astype(F)).astype(F)
        a[j0:j0 + 32] = ap
    return a


def logits64(eh, et, W1, b1, w2):
    eh, et, W1, b1, w2 = (np.asarray(v, np.float64) for v in (eh, et, W1, b1, w2))
    x = eh[:, None, :] * et[None, :, :]
    return np.maximum(x @ W1.T + b1, 0.0) @ w2.reshape(-1)


def stated_bounds(eh, et, W1, b1, w2, products):
    """(eta_a, eta', delta_s) of the derivation, float64 numpy."""
    D = 32 if eh.shape[1] <= 32 else 64
    HP = 32 if W1.shape[0] <= 32 else 64
    u = 2.0 ** -23

    def g(n):
        return n * u / (1.0 - n * u)
    eh, et, W1, b1, w2 = (np.asarray(v, np.float64) for v in (eh, et, W1, b1, w2))
    H2, T2 = np.linalg.norm(eh, axis=1).max(), np.linalg.norm(et, axis=1).max()
    Hinf, Tinf = np.abs(eh).max(), np.abs(et).max()
    Winf = np.abs(W1).max(axis=1)
    Z = np.abs(b1) + Winf * H2 * T2
    q = D * 2.0 ** -36 * Winf.max() * Hinf * Tinf
    theta3 = (g(6 * D + 1) + g(3 * D + 1)) * (1 + 2.0 ** -8) + 2.0 ** -23 + 2.0 ** -20
    theta1 = (g(6 * D + 1) + g(D + 1)) * (1 + 2.0 ** -8) + 2.0 ** -23 + 2.0 ** -10 * (1 + 2.0 ** -9)
    theta = theta1 if products == 1 else theta3
    eta_a = float((np.abs(w2.reshape(-1)) * (theta * Z + q + (HP + 4) * u * 1.01 * Z)).sum())
    return eta_a, eta_a * (1 + eta_a) + 2.0 ** -20, theta3 * H2 * T2 + D * 2.0 ** -36 * Hinf * Tinf


def _params(D, H, kind, J=64, C=96, seed=5):
    from poi_recommendation_models_amd.synthetic import init_nais_params
    P = J + C
    p = init_nais_params(P, D, H, seed=seed + D, emb_std=0.3 if kind == "normal" else 0.01, bias_std=0.1)
    eh, et = p["embed_history.weight"], p["embed_target.weight"]
    rng = np.random.default_rng(seed + 100)
    if kind == "decades":     # rows spread over five decades: every chunk and row its own scales
        for t in (eh, et):
            t *= (10.0 ** rng.uniform(-3, 2, (P, 1))).astype(F)
    if kind == "edges":
        # elements on f16 rounding midpoints ((1 + (2 m + 1) 2^-11) 2^e: a power-of-two scale keeps
        # them there) and elements 2^-27 .. 2^-33 of their row's largest (below f16's normal range
        # once the row is scaled to [2^13, 2^14)); a few W1 rows of powers of two, so A = W1 h keeps
        # the midpoints of h
        for t in (eh, et):
            m = rng.integers(0, 512, t.shape)
            e = rng.integers(-6, 0, t.shape)
            mid = ((1.0 + (2 * m + 1) * 2.0 ** -11) * 2.0 ** e * rng.choice([-1.0, 1.0], t.shape)).astype(F)
            sel = rng.random(t.shape) < 0.4
            t[sel] = mid[sel]
            big = np.abs(t).max(axis=1, keepdims=True)
            tiny = (big * 2.0 ** rng.integers(-33, -26, t.shape) * rng.choice([-1.0, 1.0], t.shape)).astype(F)
            sel = rng.random(t.shape) < 0.2
            t[sel] = tiny[sel]
        W1 = p["attn_layer1.weight"]
        W1[:4] = (2.0 ** rng.integers(-4, 0, W1[:4].shape) * rng.choice([-1.0, 1.0], W1[:4].shape)).astype(F)
    return p, J, C


def _cpu_model(p, D, H):
    from poi_recommendation_models_amd import model as M
    m = M.NAIS_basic(p["embed_history.weight"].shape[0], D, H, 0.5)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=False)
    return m.eval()


@pytest.mark.parametrize("kind", ["normal", "decades", "edges"])
@pytest.mark.parametrize("D,H", [(32, 32), (64, 64), (40, 40)])
def test_one_product_logit_within_eta_a_of_float64(D, H, kind):
    from poi_recommendation_models_amd import catalog
    p, J, C = _params(D, H, kind)
    eh, et = p["embed_history.weight"], p["embed_target.weight"]
    W1, b1, w2 = p["attn_layer1.weight"], p["attn_layer1.bias"], p["attn_layer2.weight"]
    # items: the first J rows of the history table; candidates: the last C rows of the target table
    a1 = emulate_one_product_logits(eh[:J], et[J:], W1, b1, w2).astype(np.float64)
    a64 = logits64(eh[:J], et[J:], W1, b1, w2)
    eta_a, eta, ds = stated_bounds(eh, et, W1, b1, w2, 1)
    assert np.isfinite(a1).all() and np.isfinite(eta_a) and eta_a < 0.5, eta_a
    worst = float(np.abs(a1 - a64).max())
    print("D=%d H=%d %s: eta_a %.3e, largest |a1 - a64| %.3e (%.2e of it)" % (D, H, kind, eta_a, worst, worst / eta_a))
    assert worst <= eta_a
    e1, e64 = np.exp(a1), np.exp(a64)
    assert np.all(e64 >= e1 * (1 - eta)) and np.all(e64 <= e1 * (1 + eta))
    # the function's eta' and delta_s are the stated ones (rounded upwards by 2^-20)
    w, eta_f, ds_f = catalog.ondemand_widening(_cpu_model(p, D, H), products=1)
    assert eta_f == pytest.approx(eta * (1 + 2.0 ** -20), rel=1e-12)
    assert ds_f == pytest.approx(ds * (1 + 2.0 ** -20), rel=1e-12)
    assert float(w[0]) >= eta and float(w[1]) >= ds and w.dtype == torch.float32
    # one product is the wider bound, and delta_s does not depend on it
    _, eta3_f, ds3_f = catalog.ondemand_widening(_cpu_model(p, D, H))
    assert eta_f > eta3_f and ds_f == ds3_f


def _parent_widening(model):
    """catalog.ondemand_widening as it was before the `products` argument (the three-product bound)."""
    eh, et = model._item_tables()
    w1, b1, w2 = model.attn_layer1.weight, model.attn_layer1.bias, model.attn_layer2.weight
    with torch.no_grad():
        f64 = torch.float64
        D = next((w for w in (8, 16, 32, 64, 128) if w >= w1.shape[1]), w1.shape[1])
        HP = 32 if w1.shape[0] <= 32 else 64
        u = 2.0 ** -23
        g = lambda n: n * u / (1.0 - n * u)   # noqa: E731
        H2 = torch.linalg.vector_norm(eh.to(f64), dim=1).max()
        T2 = torch.linalg.vector_norm(et.to(f64), dim=1).max()
        Hinf, Tinf = eh.abs().max().to(f64), et.abs().max().to(f64)
        Winf = w1.abs().amax(dim=1).to(f64)
        Z = b1.abs().to(f64) + Winf * H2 * T2
        q = D * 2.0 ** -36 * Winf.max() * Hinf * Tinf
        theta = (g(6 * D + 1) + g(3 * D + 1)) * (1 + 2.0 ** -8) + 2.0 ** -23 + 2.0 ** -20
        eta_a = (w2.abs().to(f64).reshape(-1) * (theta * Z + q + (HP + 4) * u * 1.01 * Z)).sum()
        eta = eta_a * (1 + eta_a) + 2.0 ** -20
        ds = theta * H2 * T2 + D * 2.0 ** -36 * Hinf * Tinf
        ok = ((Winf.max() * Hinf < 2.0 ** 100) & (Winf.max() * Hinf > 2.0 ** -100) &
              (Tinf < 2.0 ** 100) & (Tinf > 2.0 ** -100))
        both = torch.stack([eta, ds]) * (1 + 2.0 ** -20)
        both = torch.where(ok & torch.isfinite(both).all(), both, torch.full_like(both, float("inf")))
        return both.to(torch.float32), float(both[0]), float(both[1])


@pytest.mark.parametrize("kind", ["normal", "decades", "edges", "nonfinite", "clamped"])
@pytest.mark.parametrize("D,H", [(32, 32), (64, 64), (40, 40)])
def test_three_products_is_the_function_of_before_bit_for_bit(D, H, kind):
    from poi_recommendation_models_amd import catalog
    p, _, _ = _params(D, H, kind if kind in ("normal", "decades", "edges") else "normal")
    if kind == "nonfinite":
        p["embed_target.weight"][3, 1] = np.inf
    if kind == "clamped":
        p["embed_target.weight"] *= F(2.0 ** 110)
    m = _cpu_model(p, D, H)
    want = _parent_widening(m)
    for got in (catalog.ondemand_widening(m), catalog.ondemand_widening(m, products=3),
                catalog.ondemand_widening(m, 3)):
        np.testing.assert_array_equal(got[0].numpy().view(np.uint32), want[0].numpy().view(np.uint32))
        assert np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64)
        assert np.float64(got[2]).view(np.uint64) == np.float64(want[2]).view(np.uint64)
    if kind in ("nonfinite", "clamped"):   # no bound, whatever the product count
        assert not np.isfinite(want[1]) and not np.isfinite(catalog.ondemand_widening(m, products=1)[1])


def test_cache_is_keyed_on_products_and_follows_the_parameters():
    from poi_recommendation_models_amd import catalog
    p, _, _ = _params(64, 64, "normal")
    m = _cpu_model(p, 64, 64)
    w3, w1 = catalog.ondemand_widening(m), catalog.ondemand_widening(m, products=1)
    assert w1[1] > w3[1]
    assert catalog.ondemand_widening(m) is w3 and catalog.ondemand_widening(m, products=1) is w1   # hits
    with torch.no_grad():
        m.embed_history.weight.mul_(2)
    n1, n3 = catalog.ondemand_widening(m, products=1), catalog.ondemand_widening(m)
    assert n1[1] > w1[1] and n3[1] > w3[1] and n1[1] > n3[1]
    m.__dict__.pop("_widen_cache", None)                 # the documented way to drop it: both forms go
    assert catalog.ondemand_widening(m, products=1)[1] == n1[1] and catalog.ondemand_widening(m)[1] == n3[1]
    with pytest.raises(ValueError):
        catalog.ondemand_widening(m, products=2)


def test_form_choice_from_the_two_etas(monkeypatch):
    from poi_recommendation_models_amd import catalog
    f = catalog.ondemand_form
    assert f(5.65e-3, 4.2e-4) == 1                       # config 4
    assert f(2.0 ** -7, 2.0 ** -9) == 1                  # the limits are inside
    assert f(2.0 ** -7 * 1.001, 6e-4) == 3               # eta'_1 past 2^-7: three products
    assert f(3e-2, 2.0 ** -9 * 1.001) is None            # both past: split16
    assert f(float("inf"), float("inf")) is None and f(float("nan"), float("nan")) is None
    monkeypatch.setattr(catalog, "PAIR_ONDEMAND_ONE_PRODUCT", False)   # the A/B knob
    assert f(5.65e-3, 4.2e-4) == 3 and f(5.65e-3, 1e-2) is None
