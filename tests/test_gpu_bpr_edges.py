"""The fused BPR step and the BPR scorer off the beaten path: a batch of more than a thousand
triples with runs hundreds long, runs that start at every wave of a workgroup, the
user_order == NULL route, the error route, ids outside the tables in nais_bpr_forward, and
bpr.score_topk with user lists other than range(nu).

Oracle and tolerances are tests/test_gpu_bpr.py's (float64 tests/_bpr_oracle.py, _pair_E,
GRAD_RTOL, _assert_tables). The loss of n triples:
    |loss - oracle| <= sum_t (E(u,i) + E(u,j)) + 2 (n + 8) 2^-24 sum_t |term_t|
-- |d(-log sigmoid x) / dx| <= 1, so a term moves by at most its two dot-product bounds; the fp32
sum of n terms (a tree per 256, then the partials in order) adds the second part."""
import numpy as np
import pytest
import torch

import _bpr_oracle as bo
from _geoie_oracle import ulp_distance
from _helpers import GRAD_RTOL
from test_gpu_bpr import _assert_step, _assert_tables, _csr, _dev, _hists, _model, _pair_E
from poi_recommendation_models_amd import _capi, bpr
from poi_recommendation_models_amd.trainer import BPRTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tables(nu, P, D, seed):
    rng = np.random.default_rng(seed)
    return ((0.3 * rng.standard_normal((nu, D))).astype(np.float32),
            (0.3 * rng.standard_normal((P, D))).astype(np.float32))


def _empty_csr(nu, P):
    return _csr([np.zeros(0, np.int64)] * nu, P)


def _state(m):
    return (m.embed_user.weight.detach().cpu().numpy().copy(),
            m.embed_item.weight.detach().cpu().numpy().copy())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _loss_tol(U, I, uu, ii, jj, o):
    """The module docstring's bound for the batch whose oracle results are `o`."""
    terms = np.log1p(np.exp(-(o["pred_i"] - o["pred_j"])))      # -log sigmoid(x_t)
    return float(np.sum(_pair_E(U, I, uu, ii) + _pair_E(U, I, uu, jj)) +
                 2.0 * (len(uu) + 8) * 2.0 ** -24 * np.sum(np.abs(terms)))


# ------------------------------------------------------------------- (a) a large, skewed batch
N_BIG, BIG_U, BIG_P = 1030, 40, 500
HOT_USER, HOT_ITEM, ZERO_USER = 7, 11, 29
ZERO_ITEMS = np.arange(5)


def _big_batch():
    """1030 triples in a fixed shuffled order (5 loss partials, the last 6 wide; n and 2n are no
    multiples of BT_ROWS = 4): user 7 in 300 of them; item 11 the negative of 400 and the positive
    of 3; five triples with item_i == item_j, on items 0..4 that nothing else touches, two of them
    of user 29, whom nothing else touches; users 30..39 and items 5..10 and 200..499 never
    touched."""
    rng = np.random.default_rng(1030)
    n = N_BIG
    others = np.setdiff1d(np.arange(ZERO_USER), [HOT_USER])
    uu = rng.choice(others, n)
    uu[:300] = HOT_USER
    ii = rng.integers(12, 200, n)
    jj = rng.integers(12, 200, n)
    clash = ii == jj
    ii[clash] = 12 + (ii[clash] - 12 + 1) % 188
    jj[200:600] = HOT_ITEM
    ii[[610, 620, 630]] = HOT_ITEM
    same = np.array([700, 710, 720, 730, 740])
    ii[same] = jj[same] = ZERO_ITEMS
    uu[same[:2]] = ZERO_USER
    perm = rng.permutation(n)
    uu, ii, jj = uu[perm], ii[perm], jj[perm]
    assert (uu == HOT_USER).sum() == 300 and (jj == HOT_ITEM).sum() == 400 and (ii == HOT_ITEM).sum() == 3
    assert (ii == jj).sum() == 5 and len(np.setdiff1d(np.arange(BIG_U), uu)) == 10
    assert len(np.setdiff1d(np.arange(BIG_P), np.concatenate([ii, jj]))) >= 300
    return uu, ii, jj


def _fp32_in_kernel_order(U, I, uu, ii, jj, g):
    """The step's gradients restated in float32 on the host, in the kernels' order: every run of
    the stable-sorted ids summed sequentially."""
    f = np.float32
    g = g.astype(f)
    gu, gi = np.zeros_like(U), np.zeros_like(I)
    for t in np.argsort(uu, kind="stable"):
        gu[uu[t]] = gu[uu[t]] + g[t] * (I[ii[t]] - I[jj[t]])
    n = len(uu)
    keys = np.concatenate([ii, jj])
    for x in np.argsort(keys, kind="stable"):
        t, sign = (x, f(1)) if x < n else (x - n, f(-1))
        gi[keys[x]] = gi[keys[x]] + (sign * g[t]) * U[uu[t]]
    return gu, gi


# fp32 restatement against the float64 oracle, as a fraction of GRAD_RTOL max|g| (it must stay
# below 1/4 for GRAD_RTOL to be a fair bound at runs this long); measured: D = 64: user 0.0050,
# item 0.0032; D = 200: user 0.0043, item 0.0032 (max|g| about 65)
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("D", [64, 200])
def test_large_skewed_batch_against_oracle(D, wd):
    U, I = _tables(BIG_U, BIG_P, D, 40 + D)
    uu, ii, jj = _big_batch()
    n, lr = len(uu), 0.05
    o = bo.step(U, I, uu, ii, jj, lr, wd)
    gu32, gi32 = _fp32_in_kernel_order(U, I, uu, ii, jj, o["g"])
    for name, g32, g64 in (("user", gu32, o["grad_user"]), ("item", gi32, o["grad_item"])):
        ratio = np.abs(g32 - g64).max() / (GRAD_RTOL * np.abs(g64).max())
        print(f"D={D}: fp32 restatement of the {name} gradients at {ratio:.3g} of GRAD_RTOL max|g|")
        assert ratio <= 0.25
    m = _model(U, I)
    tr = BPRTrainer(m, _empty_csr(BIG_U, BIG_P), lr=lr, weight_decay=wd)
    pred, grads = {}, {}
    tr.step(_dev(uu), _dev(ii), _dev(jj), pred=pred, grads=grads)
    loss = tr.finish()
    gmax = _assert_step(o, U, I, uu, (ii, jj), None, pred, grads, lr)
    _assert_tables(m, o["embed_user"], o["embed_item"], gmax, lr)
    tol = _loss_tol(U, I, uu, ii, jj, o)
    print(f"D={D} wd={wd:g}: loss {loss!r} vs {o['loss']!r}, allowed {tol:.3g}")
    assert abs(loss - o["loss"]) <= tol
    nu, ni = _state(m)
    tu = np.setdiff1d(np.arange(BIG_U), uu)
    ti = np.setdiff1d(np.arange(BIG_P), np.concatenate([ii, jj]))
    if wd == 0.0:
        assert np.array_equal(_bits(nu[tu]), _bits(U[tu])) and np.array_equal(_bits(ni[ti]), _bits(I[ti]))
    else:
        for got, p0 in ((nu[tu], U[tu]), (ni[ti], I[ti])):
            want = (p0 - np.float32(lr) * (np.float32(wd) * p0)).astype(np.float32)
            assert ulp_distance(got, want).max() <= 1
    # rows touched only by item_i == item_j triples: the gradient is exactly +0 or -0 (x = 0, so
    # s = 0.5 and g = -0.5 exactly: the item row's +g U and -g U are exact products and cancel
    # even through the kernel's fma chain; the user row sums g * (I[i] - I[i]) = g * 0)
    gu, gi = grads["embed_user.weight"].cpu().numpy(), grads["embed_item.weight"].cpu().numpy()
    assert np.all(gu[ZERO_USER] == 0) and np.all(gi[ZERO_ITEMS] == 0)
    assert np.all(o["grad_user"][ZERO_USER] == 0) and np.all(o["grad_item"][ZERO_ITEMS] == 0)
    assert np.all(gu[tu] == 0) and np.all(gi[ti] == 0)


# ------------------------------------------------------------- (b) run placement and the bits
def _placement_batch():
    """40 triples over users >= 10 and items >= 50 with runs of length 9, 5, 2 and 1 in the user
    order and in the item order (80 keys: item 50 nine times -- 4 as a positive, 5 as a negative
    --, 51 five times, 52 twice, the rest once), in a fixed shuffled order."""
    rng = np.random.default_rng(5)
    uu = np.concatenate([[10] * 9, [11] * 5, [12] * 2, np.arange(13, 37)])
    keys = np.concatenate([[50] * 9, [51] * 5, [52] * 2, np.arange(53, 117)])
    ii = np.concatenate([keys[0:4], keys[9:12], keys[14:15], keys[16:48]])
    jj = np.concatenate([keys[4:9], keys[12:14], keys[15:16], keys[48:80]])
    assert len(uu) == len(ii) == len(jj) == 40
    uu, ii, jj = uu[rng.permutation(40)], ii[rng.permutation(40)], jj[rng.permutation(40)]
    clash = ii == jj
    assert not clash.any()
    for ids, runs in ((uu, 40), (np.concatenate([ii, jj]), 80)):
        assert sorted(np.unique(ids, return_counts=True)[1].tolist())[-3:] == [2, 5, 9] and len(ids) == runs
    return uu, ii, jj


def test_run_placement_does_not_change_bits():
    """s filler triples of smaller ids sort first and shift every run of the batch by s positions
    in the user order and by 2 s in the item order: each run starts at another wave of another
    workgroup (BT_ROWS = 4 runs per workgroup), and its sums may not depend on that."""
    D, lr = 200, 0.05
    U, I = _tables(40, 500, D, 77)
    bu, bi, bj = _placement_batch()
    rows_u, rows_i = np.unique(bu), np.unique(np.concatenate([bi, bj]))
    base = None
    for s in (0, 1, 2, 3):
        uu = np.concatenate([np.arange(s), bu])
        ii = np.concatenate([2 * np.arange(s), bi])
        jj = np.concatenate([2 * np.arange(s) + 1, bj])
        m = _model(U, I)
        tr = BPRTrainer(m, _empty_csr(40, 500), lr=lr)
        pred, grads = {}, {}
        tr.step(_dev(uu), _dev(ii), _dev(jj), pred=pred, grads=grads)
        tr.finish()
        nu, ni = _state(m)
        out = [pred["g"].cpu().numpy()[s:], grads["embed_user.weight"].cpu().numpy()[rows_u],
               grads["embed_item.weight"].cpu().numpy()[rows_i], nu[rows_u], ni[rows_i]]
        if base is None:
            base = out
            assert not np.array_equal(_bits(nu[rows_u]), _bits(U[rows_u]))        # the step applied
        for a, b in zip(out, base):
            assert np.array_equal(_bits(a), _bits(b)), s


# ----------------------------------------------------------------- (c) user_order == NULL
def _raw_step(U, I, uu, ii, jj, user_order, lr, wd):
    """nais_bpr_train_step through the C ABI from tables (U, I): (tables, grads, g, loss, err)."""
    m = _model(U, I)
    n = len(uu)
    u, i, j = _dev(uu), _dev(ii), _dev(jj)
    iorder = torch.sort(torch.cat([i, j]), stable=True)[1]
    st_u = torch.zeros(U.shape[0], dtype=torch.int32, device=DEV)
    st_i = torch.zeros(I.shape[0], dtype=torch.int32, device=DEV)
    loss, err = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    gu, gi = torch.zeros_like(m.embed_user.weight), torch.zeros_like(m.embed_item.weight)
    g = torch.empty(n, device=DEV)
    gs = _capi.NaisBPRTrainGrads()
    gs.embed_user, gs.embed_item = gu.data_ptr(), gi.data_ptr()
    lib, prm = _capi.load(), m.bpr_params()
    ws = torch.empty(lib.nais_bpr_train_step_workspace_size(prm, n), dtype=torch.uint8, device=DEV)
    _capi.check(lib.nais_bpr_train_step(
        prm, u.data_ptr(), i.data_ptr(), j.data_ptr(), n, _capi.ptr(user_order), iorder.data_ptr(), lr, wd,
        st_u.data_ptr(), st_i.data_ptr(), 1, loss.data_ptr(), err.data_ptr(), None, None, g.data_ptr(),
        gs, ws.data_ptr(), ws.numel(), _capi.stream_handle(torch.device(DEV))), "nais_bpr_train_step")
    torch.cuda.synchronize()
    return _state(m) + (gu.cpu().numpy(), gi.cpu().numpy(), g.cpu().numpy(), loss.cpu().numpy(),
                        int(err.item()))


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_null_user_order_equals_identity(wd):
    rng = np.random.default_rng(9)
    U, I = _tables(40, 500, 96, 9)
    n = 301
    uu = np.sort(rng.integers(0, 25, n))                       # grouped by ascending user, runs ~12
    ii, jj = rng.integers(0, 200, n), rng.integers(200, 400, n)
    ident = torch.arange(n, dtype=torch.int64, device=DEV)
    assert torch.equal(torch.sort(_dev(uu), stable=True)[1], ident)
    a = _raw_step(U, I, uu, ii, jj, None, 0.05, wd)
    b = _raw_step(U, I, uu, ii, jj, ident, 0.05, wd)
    assert a[-1] == 0 and b[-1] == 0
    for x, y in zip(a[:-1], b[:-1]):
        assert np.array_equal(_bits(x), _bits(y))
    assert not np.array_equal(_bits(a[0]), _bits(U))            # and the step applied
    o = bo.step(U, I, uu, ii, jj, 0.05, wd)                     # the NULL route is also right
    for got, ref in ((a[2], o["grad_user"]), (a[3], o["grad_item"])):
        assert np.all(np.abs(got - ref) <= GRAD_RTOL * np.abs(ref).max())


# --------------------------------------------------------------------------- (d) the error route
@pytest.mark.parametrize("field,pos,value", [("item_j", 10, "P"), ("user", 280, -1), ("item_i", 256, -1)])
def test_error_route(field, pos, value):
    """One id of 300 triples is outside its table (in the first or the second workgroup of 256 of
    the forward kernel, which bounds-checks before any access): err |= 2, the loss of the valid
    triples is still reported, no table is written by this step or the next, finish() raises and
    clears the flag, and the step after that applies."""
    nu, P, D, lr, wd = 40, 500, 64, 0.05, 1e-3
    U, I = _tables(nu, P, D, 31)
    rng = np.random.default_rng(31)
    n = 300
    uu, ii, jj = rng.integers(0, 30, n), rng.integers(0, 250, n), rng.integers(250, P, n)
    bu, bi, bj = (a.copy() for a in (uu, ii, jj))
    {"user": bu, "item_i": bi, "item_j": bj}[field][pos] = P if value == "P" else value
    m = _model(U, I)
    tr = BPRTrainer(m, _empty_csr(nu, P), lr=lr, weight_decay=wd)
    ok = np.arange(n) != pos
    o_ok = bo.step(U, I, uu[ok], ii[ok], jj[ok], lr, wd)
    tol_ok = _loss_tol(U, I, uu[ok], ii[ok], jj[ok], o_ok)

    tr.step(_dev(bu), _dev(bi), _dev(bj))
    l1 = float(tr.loss_sum.item())
    assert int(tr._err.item()) == 2
    assert abs(l1 - o_ok["loss"]) <= tol_ok
    for got, ref in zip(_state(m), (U, I)):
        assert np.array_equal(_bits(got), _bits(ref))

    o = bo.step(U, I, uu, ii, jj, lr, wd)
    tol = _loss_tol(U, I, uu, ii, jj, o)
    tr.step(_dev(uu), _dev(ii), _dev(jj))                       # valid, but the flag is still up
    l2 = float(tr.loss_sum.item())
    assert abs((l2 - l1) - o["loss"]) <= tol + 2.0 ** -23 * abs(l2)      # + the rounding of l1 + loss
    for got, ref in zip(_state(m), (U, I)):
        assert np.array_equal(_bits(got), _bits(ref))

    with pytest.raises(RuntimeError):
        tr.finish()
    assert int(tr._err.item()) == 0
    pred, grads = {}, {}
    tr.step(_dev(uu), _dev(ii), _dev(jj), pred=pred, grads=grads)
    gmax = _assert_step(o, U, I, uu, (ii, jj), None, pred, grads, lr)
    _assert_tables(m, o["embed_user"], o["embed_item"], gmax, lr)
    l3 = tr.finish()
    assert abs((l3 - l2) - o["loss"]) <= tol + 2.0 ** -23 * abs(l3)


# ------------------------------------------------- (e) nais_bpr_forward with ids outside the tables
def _raw_forward(m, u, i, j):
    n = u.numel()
    oi = torch.full((n,), 123.0, device=DEV)
    oj = torch.full((n,), 123.0, device=DEV) if j is not None else None
    _capi.check(_capi.load().nais_bpr_forward(
        m.bpr_params(), u.data_ptr(), i.data_ptr(), _capi.ptr(j), n, oi.data_ptr(), _capi.ptr(oj),
        _capi.stream_handle(torch.device(DEV))), "nais_bpr_forward")
    torch.cuda.synchronize()
    return oi.cpu().numpy(), (oj.cpu().numpy() if j is not None else None)


def test_forward_ids_outside_the_tables_give_nan():
    nu, P, D, n = 40, 500, 33, 300
    U, I = _tables(nu, P, D, 12)
    m = _model(U, I)
    rng = np.random.default_rng(12)
    uu, ii, jj = rng.integers(0, nu, n), rng.integers(0, P, n), rng.integers(0, P, n)
    uu[[3, 257]] = [-1, nu]                                     # the kernel checks before it reads
    ii[[40, 258, 299]] = [-1, P, P]
    jj[[41, 3, 255]] = [P, 5, -1]
    bad_u = (uu < 0) | (uu >= nu)
    bad_i, bad_j = bad_u | (ii < 0) | (ii >= P), bad_u | (jj < 0) | (jj >= P)
    assert bad_u.sum() == 2 and bad_i.sum() == 5 and bad_j.sum() == 4
    u, i, j = _dev(uu), _dev(ii), _dev(jj)
    oi, oj = _raw_forward(m, u, i, j)
    assert np.array_equal(np.isnan(oi), bad_i) and np.array_equal(np.isnan(oj), bad_j)
    oi1, none = _raw_forward(m, u, i, None)                      # item_j = NULL, out_j = NULL
    assert none is None and np.array_equal(np.isnan(oi1), bad_i)
    with torch.no_grad():
        good = ~(bad_i | bad_j)
        pi, pj = m(_dev(uu[good]), _dev(ii[good]), _dev(jj[good]))
        assert np.array_equal(_bits(oi[good]), _bits(pi.cpu().numpy()))
        assert np.array_equal(_bits(oj[good]), _bits(pj.cpu().numpy()))
        assert np.array_equal(_bits(oi1[good]), _bits(pi.cpu().numpy()))
        only_i, only_j = ~bad_i & bad_j, ~bad_j & bad_i            # one side valid: that side is right
        pi2, _ = m(_dev(uu[only_i]), _dev(ii[only_i]), _dev(ii[only_i]))
        assert np.array_equal(_bits(oi[only_i]), _bits(pi2.cpu().numpy()))
        pj2, _ = m(_dev(uu[only_j]), _dev(jj[only_j]), _dev(jj[only_j]))
        assert np.array_equal(_bits(oj[only_j]), _bits(pj2.cpu().numpy()))
    with pytest.raises(IndexError):                                # the module itself refuses such ids
        m(u, i, j)


# ------------------------------------------------------------- (f) score_topk with a real user list
@pytest.fixture(scope="module")
def topk_case():
    rng = np.random.default_rng(80)
    U, I = _tables(80, 5003, 20, 80)
    I[1000:1040] = I[999]                                        # exact ties, so the id order matters
    hists = _hists(rng, 80, 5003, 50)
    m, X = _model(U, I), _csr(hists, 5003)
    _, _, keys, cnt = bpr.score_topk(m, X, range(80), 50, num_chunks=1, return_keys=True)
    return m, X, keys.cpu().numpy(), cnt.cpu().numpy()


_SUBSET = np.random.default_rng(33).permutation(np.arange(1, 80))[:33]
_REPEATED = np.random.default_rng(70).permutation(np.setdiff1d(np.arange(80), [17]))[:70]
_REPEATED[[3, 30, 40, 63, 69]] = 17                              # tiles of 32 users: 0, 0, 1, 1, 2
USER_LISTS = {"reversed": np.arange(79, -1, -1), "subset": _SUBSET, "repeated": _REPEATED,
              "single": np.array([41])}


@pytest.mark.parametrize("num_chunks", [1, 3])
@pytest.mark.parametrize("name", list(USER_LISTS))
def test_score_topk_follows_the_user_list(topk_case, name, num_chunks):
    m, X, ref_keys, ref_cnt = topk_case
    users = USER_LISTS[name]
    assert name != "subset" or (0 not in users and len(users) == 33)
    ids, sc, keys, cnt = bpr.score_topk(m, X, users, 50, num_chunks=num_chunks, return_keys=True)
    keys, cnt = keys.cpu().numpy(), cnt.cpu().numpy()
    assert keys.shape == (len(users), 50)
    assert np.array_equal(cnt, ref_cnt[users])
    live = np.arange(50)[None, :] < cnt[:, None]
    assert np.array_equal(np.where(live, keys, 0), np.where(live, ref_keys[users], 0))
    assert len(set(ref_cnt.tolist())) > 1 and ref_cnt.max() == 50   # short and full lists both occur
