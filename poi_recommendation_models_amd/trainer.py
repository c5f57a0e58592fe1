"""The NAIS training loops of run.py on the device (SURVEY.md 8(f1) + 8(f2)): NAIS_basic
(run.py:91-111), NAIS_regionEmbedding (run.py:139-200), NAIS_region_distance_Embedding
(run.py:206-262) and NAIS_distance_Embedding (run.py:365-430).

    for buid in shuffled users:                                   run.py:96-99
        user_history, train_data, train_label = get_NAIS_batch(...)   batches.py:24-50  -> GPU
        optimizer.zero_grad(); prediction = model(...)            run.py:102-103
        loss = model.loss_func(...); loss.backward()              run.py:104-105     -> 1 call
        train_loss += loss.item(); optimizer.step()               run.py:107-109

`NAISTrainer.epoch(users)` runs that loop with two C-ABI calls per user -- `nais_make_train_batch`
(device-side negative sampling) and `nais_train_step` (forward, BCELoss, backward, Adagrad) --
and one host sync per epoch (the reference syncs on loss.item() every user). The region /
distance variants build get_NAIS_batch_region's extra inputs (batches.py:67-108) on the device too
-- the region ids of the history and target rows, and for the distance variants the
target_lat_long rows of run.py:240-245 (|coordinate differences| in float64, as latlon_mat holds
them, cast to float32) -- and step through `nais_train_step_ex`, which also updates embed_region /
dist_layer (torch.optim.Adagrad over model.parameters(), run.py:155, 222). The model's
parameters are updated in place; Adagrad's accumulators live in the trainer with torch's
semantics (state 'sum' and 'step' per parameter, `optimizer_state()` exports them).

The per-step arithmetic is the drop-in path's (NAIS_basic train-mode forward + backward +
optim.Adagrad), differing only in fp32 summation order; tests/test_gpu_train.py checks both
against the oracle. Batches follow get_NAIS_batch's distribution (shuffled positives as the
shared history, num_ng distinct uniform negatives per positive), not Python's random stream.

`GeoIETrainer` is the same treatment of train_GeoIE (run.py:687-715): `nais_geoie_make_train_batch`
is get_GeoIE_batch (batches.py:204-242) on the device and `nais_geoie_train_step` is forward,
loss_function, backward and torch.optim.SGD in place on the four embedding tables.

`BPRTrainer` is train_BPR's loop (run.py:490-509): `nais_bpr_make_train_batch` is get_BPR_batch
(batches.py:6-22) for a whole list of users and `nais_bpr_train_step` is forward, the BPR loss,
backward and torch.optim.SGD in place on both tables, deterministic (no float atomics).

`New1Trainer` is train_NAIS_new's loop (run_new.py:391-410): `nais_new1_make_train_batch` is
trainDataset.__getitem__ (run_new.py:107-137) on the device and `nais_new1_train_step` is forward,
nn.BCELoss, backward and torch.optim.Adam (dense, with weight decay) in place on the five
parameter tensors, deterministic.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch
from torch.autograd.graph import increment_version

from . import _capi
from .catalog import device_csr


class NAISTrainer:
    def __init__(self, model, train_matrix, lr=0.01, lr_decay=0.0, weight_decay=0.0, eps=1e-10,
                 initial_accumulator_value=0.0, num_ng=4, region_of=None, poi_coords=None):
        """region_of: businessRegionEmbedList (POI -> region id, run.py:148-151) for the region
        variants; poi_coords: [P, 2] (lat, lng) for the distance variants (latlon_mat's source,
        run.py:47-54)."""
        from .model import (NAIS_basic, NAIS_distance_Embedding, NAIS_region_distance_Embedding,
                            NAIS_regionEmbedding)
        if not isinstance(model, (NAIS_basic, NAIS_regionEmbedding, NAIS_region_distance_Embedding,
                                  NAIS_distance_Embedding)):
            raise NotImplementedError(f"NAISTrainer: {type(model).__name__} has no device training step")
        dev = model._check_device()
        self.region = model.VARIANT in (_capi.VARIANT_REGION, _capi.VARIANT_REGION_DISTANCE)
        self.distance = model.VARIANT in (_capi.VARIANT_REGION_DISTANCE, _capi.VARIANT_DISTANCE)
        if self.region and region_of is None:
            raise ValueError(f"{type(model).__name__}: NAISTrainer needs region_of (businessRegionEmbedList)")
        if self.distance and poi_coords is None:
            raise ValueError(f"{type(model).__name__}: NAISTrainer needs poi_coords")
        self.region_of = (torch.as_tensor(np.asarray(region_of, dtype=np.int64)).to(dev)
                          if self.region else None)
        self.coords = (torch.as_tensor(np.ascontiguousarray(poi_coords, dtype=np.float64)).to(dev)
                       if self.distance else None)
        self.model, self.dev = model, dev
        self.csr = device_csr(train_matrix, dev)
        self.num_ng = int(num_ng)
        self.lr, self.lr_decay, self.weight_decay, self.eps = lr, lr_decay, weight_decay, eps
        self.step_count = 0
        ps = dict(model.named_parameters())
        self._names = ["embed_history.weight", "embed_target.weight", "attn_layer1.weight",
                       "attn_layer1.bias", "attn_layer2.weight"]
        if self.region:
            self._names.append("embed_region.weight")
        if self.distance:
            self._names += ["dist_layer.weight", "dist_layer.bias"]
        self.sums = {k: torch.full_like(ps[k], initial_accumulator_value) for k in self._names}
        P, D = ps["embed_history.weight"].shape
        H, DIN = ps["attn_layer1.weight"].shape
        self._g_eh = torch.zeros(P, D, device=dev)
        self._g_et = torch.zeros(P, D, device=dev)
        self._g_small = torch.zeros(H * DIN + 2 * H, device=dev)
        self._g_er = torch.zeros_like(ps["embed_region.weight"]) if self.region else None
        self._g_dist = torch.zeros(6, device=dev) if self.distance else None
        self._st_eh = torch.zeros(P, dtype=torch.int32, device=dev)
        self._st_et = torch.zeros(P, dtype=torch.int32, device=dev)
        self.loss_sum = torch.zeros(1, device=dev)
        self.bad_rows = torch.zeros(1, dtype=torch.int32, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        self._bufs = {}

    # ------------------------------------------------------------------ batches (f2)
    def batch(self, uid, seed=None):
        """get_NAIS_batch(train_matrix, P, uid, num_ng) on the device: (hist [n], target [b],
        labels [b]); the reference's user_history is hist repeated b times. Region variants:
        + (hist_region [n], target_region [b]) as get_NAIS_batch_region (batches.py:67-108);
        distance variants: + target_lat_long [b, n, 2] f32 (run.py:240-245)."""
        n = int(self.csr.hist_len[uid])
        b = n * (1 + self.num_ng)
        key = (n, b)
        if key not in self._bufs:
            self._bufs = {key: (torch.empty(n, dtype=torch.int64, device=self.dev),
                                torch.empty(b, dtype=torch.int64, device=self.dev),
                                torch.empty(b, dtype=torch.float32, device=self.dev))}
        hist, tgt, lab = self._bufs[key]
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        lib = _capi.load()
        _capi.check(lib.nais_make_train_batch(self.csr.indptr.data_ptr(), self.csr.indices.data_ptr(),
                                              int(uid), n, self.csr.shape[1], self.num_ng, seed,
                                              hist.data_ptr(), tgt.data_ptr(), lab.data_ptr(),
                                              self._err.data_ptr(),
                                              _capi.stream_handle(self.dev)), "nais_make_train_batch")
        out = (hist, tgt, lab)
        if self.region:       # businessRegionEmbedList[positives] / [train_data] (batches.py:96-101)
            out += (self.region_of.index_select(0, hist), self.region_of.index_select(0, tgt))
        if self.distance:
            out += (self.lat_long(hist, tgt),)
        return out

    def lat_long(self, hist, target):
        """target_lat_long [b, n, 2] f32 = latlon_mat[target, hist] (run.py:240-245): the absolute
        float64 coordinate differences of lat_lon_mat (run.py:47-54), cast to float32."""
        c = self.coords
        return (c.index_select(0, target)[:, None, :] - c.index_select(0, hist)[None, :, :]).abs_().to(
            torch.float32)

    # ------------------------------------------------------------------ one step (f1)
    def _opt_struct(self):
        o = _capi.NaisAdagradState()
        o.lr, o.lr_decay, o.weight_decay, o.eps = self.lr, self.lr_decay, self.weight_decay, self.eps
        o.step = self.step_count
        s = self.sums
        o.sum_embed_history = s["embed_history.weight"].data_ptr()
        o.sum_embed_target = s["embed_target.weight"].data_ptr()
        o.sum_w1 = s["attn_layer1.weight"].data_ptr()
        o.sum_b1 = s["attn_layer1.bias"].data_ptr()
        o.sum_w2 = s["attn_layer2.weight"].data_ptr()
        o.grad_embed_history = self._g_eh.data_ptr()
        o.grad_embed_target = self._g_et.data_ptr()
        o.grad_small = self._g_small.data_ptr()
        o.stamp_embed_history = self._st_eh.data_ptr()
        o.stamp_embed_target = self._st_et.data_ptr()
        return o

    def step(self, hist, target, labels, *side, dropout_seed=None, pred=None):
        """One fused step on a get_NAIS_batch batch given as the shared history hist [n] (or the
        reference's [b, n] user_history), target [b], labels [b]; `side` = what batch() adds for
        the variant: (hist_region, target_region) for the region variants ([n] or the reference's
        [b, n]), then target_lat_long [b, n, 2] for the distance variants."""
        m = self.model
        if hist.dim() == 2:
            hist = hist[0] if hist.shape[0] else hist.new_empty(0)
        hist = hist.to(torch.int64).contiguous()
        target = target.to(torch.int64).contiguous()
        labels = labels.to(torch.float32).contiguous()
        b, n = target.numel(), hist.numel()
        want = 2 * self.region + self.distance
        if len(side) != want:
            raise TypeError(f"{type(m).__name__}: step() takes {want} side input(s) after labels")
        sd = _capi.NaisTrainSide()
        keep = []
        if self.region:
            hreg, treg = side[0], side[1]
            if hreg.dim() == 2:
                hreg = hreg[0] if hreg.shape[0] else hreg.new_empty(0)
            hreg = hreg.to(torch.int64).contiguous()
            treg = treg.to(torch.int64).contiguous()
            keep += [hreg, treg]
            sd.hist_region, sd.target_region = _capi.ptr(hreg), _capi.ptr(treg)
        if self.distance:
            ll = side[-1].to(torch.float32)
            if tuple(ll.shape) != (b, n, 2):
                raise ValueError("target_lat_long must be [b, n, 2]")
            if not (ll.stride(2) == 1 and ll.stride(1) == 2):
                ll = ll.contiguous()
            keep.append(ll)
            sd.target_lat_long, sd.latlon_ld = ll.data_ptr(), ll.stride(0)
        drop = getattr(m, "drop", None)        # none in the two distance variants (model.py:268, 369)
        p = float(drop.p) if drop is not None and m.training else 0.0
        if dropout_seed is None:
            dropout_seed = int(torch.randint(0, 2**62, (1,)).item())
        self.step_count += 1
        lib = _capi.load()
        prm = m.nais_params()
        need = lib.nais_train_step_workspace_size(prm, b, n)
        if self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=self.dev)
        args = (_capi.ptr(hist) if n else None, n, _capi.ptr(target) if b else None,
                _capi.ptr(labels) if b else None, b, p, dropout_seed, self.loss_sum.data_ptr(),
                self.bad_rows.data_ptr(), _capi.ptr(pred), self._ws.data_ptr(), self._ws.numel(),
                _capi.stream_handle(self.dev))
        if not (self.region or self.distance):
            _capi.check(lib.nais_train_step(prm, self._opt_struct(), *args), "nais_train_step")
            self._bump_versions()
            return
        os_ = _capi.NaisAdagradSide()
        if self.region:
            os_.sum_embed_region = self.sums["embed_region.weight"].data_ptr()
            os_.grad_embed_region = self._g_er.data_ptr()
        if self.distance:
            os_.sum_dist_w = self.sums["dist_layer.weight"].data_ptr()
            os_.sum_dist_b = self.sums["dist_layer.bias"].data_ptr()
            os_.grad_dist = self._g_dist.data_ptr()
        _capi.check(lib.nais_train_step_ex(prm, sd, self._opt_struct(), os_, *args), "nais_train_step_ex")
        self._bump_versions()
        del keep

    def _bump_versions(self):
        """The fused step writes the parameters through raw pointers: bump their version counters
        as an in-place torch op would, so version-keyed caches (model._score_params' padded copies
        for embed widths off the kernels' native set) are rebuilt before the next scoring call."""
        for q in self.model.parameters():
            increment_version(q)

    def epoch(self, users=None, shuffle=True):
        """One pass of run.py:96-109 over `users` (default: every user, shuffled as run.py:96-97).
        Returns train_loss (the sum of the per-user mean BCE losses, run.py:107)."""
        if users is None:
            users = np.arange(self.csr.shape[0])
        users = np.asarray(users, dtype=np.int64)
        if shuffle:
            users = users[torch.randperm(len(users)).numpy()]
        self.model.train()
        self.loss_sum.zero_()
        P = self.csr.shape[1]
        for u in users.tolist():
            n = int(self.csr.hist_len[u])
            if n == 0:
                continue   # empty batch: the reference's step changes nothing
            if n * (1 + self.num_ng) > P:
                raise ValueError(f"user {u}: {n} positives x {1 + self.num_ng} rows exceed {P} POIs "
                                 "(get_NAIS_batch cannot draw enough negatives)")
            self.step(*self.batch(u))
        return self.finish()

    def finish(self):
        """Host sync: the accumulated loss; raises like the reference's BCELoss if a batch had a
        NaN prediction (its update and all later ones were skipped)."""
        bad = int(self.bad_rows.item())
        if bad:
            raise RuntimeError(f"all elements of input should be between 0 and 1 ({bad} NaN "
                               "predictions: a single-item history equal to its target, "
                               "model.py:92-95); the updates from that batch on were skipped")
        if int(self._err.item()):
            raise RuntimeError("nais_make_train_batch: history length disagrees with the CSR")
        return float(self.loss_sum.item())

    def optimizer_state(self):
        """torch.optim.Adagrad-style per-parameter state {name: {'step', 'sum'}}."""
        return {k: {"step": torch.tensor(float(self.step_count)), "sum": self.sums[k]}
                for k in self._names}


class GeoIETrainer:
    """train_GeoIE's loop (run.py:687-715) on the device: `batch()` is get_GeoIE_batch
    (batches.py:204-242), `step()` is run.py:705-715 (forward, loss_function, backward,
    torch.optim.SGD(lr, weight_decay) without momentum) updating the model's four tables in
    place, `epoch()` the loop with one host sync at its end. Distances come from exactly one of
    `dist_mat` (the reference's P x P matrix, run.py:683) and `poi_coords` ([P, 2] lat / lng)."""

    def __init__(self, model, train_matrix, lr=0.01, weight_decay=0.0, num_ng=4, dist_mat=None,
                 poi_coords=None):
        from .geoie import _distance_source
        from .model import GeoIE
        if not isinstance(model, GeoIE):
            raise NotImplementedError(f"GeoIETrainer: {type(model).__name__} is not GeoIE")
        dev = model._check_device()
        if int(num_ng) < 1:
            raise ValueError(f"GeoIETrainer: num_ng must be at least 1, got {num_ng}")
        if (dist_mat is None) == (poi_coords is None):
            raise ValueError("GeoIETrainer needs exactly one of dist_mat and poi_coords")
        self.model, self.dev = model, dev
        self.csr = device_csr(train_matrix, dev)
        P = model.POI_count
        if self.csr.shape[1] != P:
            raise ValueError(f"train_matrix has {self.csr.shape[1]} POIs, model has {P}")
        self.coords, self.dist_mat = _distance_source(dev, P, dist_mat, poi_coords)
        X = train_matrix.tocsr() if not hasattr(train_matrix, "indptr") else train_matrix
        if not X.has_sorted_indices:   # the order device_csr holds the rows in
            X = X.sorted_indices()
        self.data = torch.from_numpy(np.asarray(X.data, dtype=np.float64)).to(dev)
        self.num_ng, self.lr, self.weight_decay = int(num_ng), float(lr), float(weight_decay)
        self.step_count = 0
        self._st_t = torch.zeros(P, dtype=torch.int32, device=dev)
        self._st_h = torch.zeros(P, dtype=torch.int32, device=dev)
        self.loss_sum = torch.zeros(1, device=dev)
        self.bad_rows = torch.zeros(1, dtype=torch.int32, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        self._bufs = {}

    def _check_user(self, uid):
        h = int(self.csr.hist_len[uid])
        if h == 0:   # the reference's reshape raises here (model.py:798)
            raise ValueError(f"GeoIE: empty history (user {int(uid)})")
        P = self.csr.shape[1]
        if h * self.num_ng > P - h:
            raise ValueError(f"user {int(uid)}: {h} positives x {self.num_ng} negatives exceed the "
                             f"{P - h} POIs outside the history (get_GeoIE_batch cannot draw them)")
        return h

    def batch(self, uid, seed=None):
        """get_GeoIE_batch(train_matrix, P, P, uid, num_ng, dist_mat) on the device: (user_id [b],
        hist [h], target [b], labels [b], freq [b, 1] int64, distances [b, h] f32); the reference's
        user_history is hist repeated b times. The buffers are reused by the next call of the
        same shape."""
        h = self._check_user(uid)
        b = h * (1 + self.num_ng)
        if h not in self._bufs:
            d = self.dev
            self._bufs = {h: (torch.empty(b, dtype=torch.int64, device=d),
                              torch.empty(h, dtype=torch.int64, device=d),
                              torch.empty(b, dtype=torch.int64, device=d),
                              torch.empty(b, dtype=torch.float32, device=d),
                              torch.empty(b, 1, dtype=torch.int64, device=d),
                              torch.empty(b, h, dtype=torch.float32, device=d))}
        uidt, hist, tgt, lab, freq, dist = self._bufs[h]
        uidt.fill_(int(uid))
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        _capi.check(_capi.load().nais_geoie_make_train_batch(
            self.csr.indptr.data_ptr(), self.csr.indices.data_ptr(), self.data.data_ptr(), int(uid), h,
            self.csr.shape[1], self.num_ng, seed, _capi.ptr(self.coords), _capi.ptr(self.dist_mat),
            hist.data_ptr(), tgt.data_ptr(), lab.data_ptr(), freq.data_ptr(), dist.data_ptr(), h,
            self._err.data_ptr(), _capi.stream_handle(self.dev)), "nais_geoie_make_train_batch")
        return uidt, hist, tgt, lab, freq, dist

    def step(self, user_id, hist, target, labels, freq, distances, pred=None, grads=None):
        """One fused step (run.py:705-715) on a batch as batch() returns it, or in the reference's
        own layout (get_GeoIE_batch: user_history [b, h] repeated rows, user_id [b]). `pred`:
        optional [b] f32 output; `grads`: optional dict that receives the four row-gradient blocks
        under the parameter names (UserPreference.weight [D], PoiPreference.weight [b, D],
        GeoSusceptibility.weight [b, D], GeoInfluence.weight [h, D], rows in batch order)."""
        m = self.model
        on_dev = isinstance(user_id, torch.Tensor)
        dev = m._check_device(user_id if on_dev else None, hist, target, labels, freq, distances)
        if hist.dim() == 2:
            hist = hist[0] if hist.shape[0] else hist.new_empty(0)
        uids = torch.unique(user_id.reshape(-1)).tolist() if on_dev else [int(user_id)]
        if len(uids) != 1:
            raise ValueError(f"GeoIETrainer.step: one batch is one user, got users {uids}")
        hist = hist.reshape(-1).to(torch.int64).contiguous()
        target = target.reshape(-1).to(torch.int64).contiguous()
        labels = labels.reshape(-1).to(torch.float32).contiguous()
        freq = freq.reshape(-1).to(torch.int64).contiguous()
        b, h = target.numel(), hist.numel()
        if h == 0:
            raise ValueError(f"GeoIE: empty history (user {uids[0]})")
        distances = distances.to(torch.float32)
        if tuple(distances.shape) != (b, h) or labels.numel() != b or freq.numel() != b or b == 0:
            raise ValueError(f"labels / freq must hold b = {b} rows (b >= 1) and distances [b, h = {h}]; "
                             f"got {labels.numel()}, {freq.numel()}, {tuple(distances.shape)}")
        if distances.stride(1) != 1:
            distances = distances.contiguous()
        D = int(m.emb_dimension)
        gs = _capi.NaisGeoIETrainGrads()
        if grads is not None:
            gu = torch.empty(D, device=dev)
            gp, gh = torch.empty(b, D, device=dev), torch.empty(b, D, device=dev)
            gg = torch.empty(h, D, device=dev)
            grads.update({"UserPreference.weight": gu, "PoiPreference.weight": gp,
                          "GeoSusceptibility.weight": gh, "GeoInfluence.weight": gg})
            gs.user_pref, gs.poi_pref = gu.data_ptr(), gp.data_ptr()
            gs.geo_suscept, gs.geo_influence = gh.data_ptr(), gg.data_ptr()
        if pred is not None and (pred.dtype != torch.float32 or pred.numel() != b or not pred.is_contiguous()):
            raise ValueError("pred must be a contiguous float32 tensor of b elements")
        lib = _capi.load()
        prm = m.geoie_params()
        need = lib.nais_geoie_train_step_workspace_size(prm, b, h)
        if self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=dev)
        self.step_count += 1
        _capi.check(lib.nais_geoie_train_step(
            prm, int(uids[0]), hist.data_ptr(), h, target.data_ptr(), labels.data_ptr(), freq.data_ptr(),
            b, distances.data_ptr(), distances.stride(0), self.lr, self.weight_decay,
            self._st_t.data_ptr(), self._st_h.data_ptr(), self.step_count, self.loss_sum.data_ptr(),
            self.bad_rows.data_ptr(), self._err.data_ptr(), _capi.ptr(pred),
            gs if grads is not None else None, self._ws.data_ptr(), self._ws.numel(),
            _capi.stream_handle(dev)), "nais_geoie_train_step")
        self._bump_versions()

    def _step_uid(self, uid, batch):
        """step() on a batch() result: the user is known, so no device read of user_id."""
        return self.step(int(uid), *batch[1:])

    def _bump_versions(self):
        """As NAISTrainer._bump_versions: the step writes through raw pointers."""
        for q in self.model.parameters():
            increment_version(q)

    def epoch(self, users=None, shuffle=True):
        """run.py:694-715 over `users` (default: every user, shuffled as run.py:694-696). Returns
        train_loss (run.py:714), read with the epoch's one host sync."""
        if users is None:
            users = np.arange(self.csr.shape[0])
        users = np.asarray(users, dtype=np.int64)
        if shuffle:
            users = users[torch.randperm(len(users)).numpy()]
        self.model.train()
        self.loss_sum.zero_()
        for u in users.tolist():
            self._step_uid(u, self.batch(u))
        return self.finish()

    def finish(self):
        """Host sync: the accumulated loss. Raises if a step saw a repeated target or history
        entry, an id outside the catalog, or a history length that disagrees with the CSR (that
        step and every later one left the tables untouched); warns if a loss term was not finite
        (the reference prints its tensors and carries on, model.py:820-826)."""
        err = int(self._err.item())
        if err:
            self._err.zero_()
            raise RuntimeError("GeoIETrainer: a batch had a repeated target or history entry, an id "
                               "outside the catalog, or a history length that disagrees with the CSR "
                               f"(code {err}); that step and the later ones were not applied")
        bad = int(self.bad_rows.item())
        if bad:
            self.bad_rows.zero_()
            warnings.warn(f"GeoIE: {bad} row(s) with a non-finite loss term (model.py:820)", RuntimeWarning)
        return float(self.loss_sum.item())


class BPRTrainer:
    """train_BPR's loop (run.py:490-509) on the device: `batch()` is get_BPR_batch
    (batches.py:6-22) for a list of users, `step()` is run.py:504-509 (forward, the loss
    -sum(log(sigmoid(pred_i - pred_j))), backward, torch.optim.SGD(lr, weight_decay) without
    momentum) updating both embedding tables in place, `epoch()` the loop with one host sync at
    its end. A step is deterministic: the same batch from the same state gives the same bits."""

    def __init__(self, model, train_matrix, lr=0.01, weight_decay=0.0):
        from .model import BPR
        if not isinstance(model, BPR):
            raise NotImplementedError(f"BPRTrainer: {type(model).__name__} is not BPR")
        dev = model._check_device()
        self.model, self.dev = model, dev
        self.csr = device_csr(train_matrix, dev)
        if self.csr.shape[1] != model.POI_count or self.csr.shape[0] > model.user_num:
            raise ValueError(f"train_matrix is {self.csr.shape}, model has {model.user_num} users "
                             f"and {model.POI_count} POIs")
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.step_count = 0
        self._st_u = torch.zeros(model.user_num, dtype=torch.int32, device=dev)
        self._st_i = torch.zeros(model.POI_count, dtype=torch.int32, device=dev)
        self.loss_sum = torch.zeros(1, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)

    def batch(self, user_ids, seed=None):
        """get_BPR_batch(train_matrix, P, user_ids) on the device: (user, item_i, item_j), int64
        [n] each, n = the users' history lengths summed. Per user the positives in CSR order and
        as many distinct negatives drawn uniformly from outside the history; triples are grouped
        by user (the reference's final shuffle only changes the summation order). A user with
        more positives than POIs outside its history raises ValueError (the reference's
        negative[i] raises IndexError there)."""
        users = np.asarray(list(user_ids) if not isinstance(user_ids, np.ndarray) else user_ids,
                           dtype=np.int64).reshape(-1)
        if len(users) and (users.min() < 0 or users.max() >= self.csr.shape[0]):
            raise IndexError("BPRTrainer.batch: user id out of range")
        hl = self.csr.hist_len[users] if len(users) else np.zeros(0, np.int64)
        P = self.csr.shape[1]
        if np.any(hl > P - hl):
            u = int(users[np.argmax(hl > P - hl)])
            raise ValueError(f"user {u}: {int(self.csr.hist_len[u])} positives exceed the "
                             f"{P - int(self.csr.hist_len[u])} POIs outside the history "
                             "(get_BPR_batch cannot draw them)")
        off = np.zeros(len(users), dtype=np.int64)
        if len(users):
            off[1:] = np.cumsum(hl)[:-1]
        n = int(hl.sum())
        d = self.dev
        user = torch.empty(n, dtype=torch.int64, device=d)
        item_i = torch.empty(n, dtype=torch.int64, device=d)
        item_j = torch.empty(n, dtype=torch.int64, device=d)
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        if n:
            users_d, off_d = torch.from_numpy(users).to(d), torch.from_numpy(off).to(d)   # both alive
            _capi.check(_capi.load().nais_bpr_make_train_batch(
                self.csr.indptr.data_ptr(), self.csr.indices.data_ptr(), self.csr.shape[0], users_d.data_ptr(),
                off_d.data_ptr(), len(users), P, seed, user.data_ptr(), item_i.data_ptr(), item_j.data_ptr(),
                self._err.data_ptr(), _capi.stream_handle(d)), "nais_bpr_make_train_batch")
        return user, item_i, item_j

    def step(self, user, item_i, item_j, pred=None, grads=None):
        """One fused step (run.py:504-509) on n triples, in any order (batch()'s, or the
        reference's shuffled get_BPR_batch). `pred`: optional dict that receives prediction_i /
        prediction_j / g ([n] f32 each); `grads`: optional dict that receives the dense gradients
        under the parameter names (embed_user.weight [U, D], embed_item.weight [P, D])."""
        m = self.model
        dev = m._check_device(user, item_i, item_j)
        user = user.reshape(-1).to(torch.int64).contiguous()
        item_i = item_i.reshape(-1).to(torch.int64).contiguous()
        item_j = item_j.reshape(-1).to(torch.int64).contiguous()
        n = user.numel()
        if item_i.numel() != n or item_j.numel() != n or n == 0:
            raise ValueError(f"user, item_i and item_j must hold the same n >= 1 triples; got "
                             f"{n}, {item_i.numel()}, {item_j.numel()}")
        # the stable orders the step sums in (plumbing; the sums themselves are the kernels')
        uorder = torch.sort(user, stable=True)[1]
        iorder = torch.sort(torch.cat([item_i, item_j]), stable=True)[1]
        gs = _capi.NaisBPRTrainGrads()
        if grads is not None:
            gu = torch.zeros_like(m.embed_user.weight)
            gi = torch.zeros_like(m.embed_item.weight)
            grads.update({"embed_user.weight": gu, "embed_item.weight": gi})
            gs.embed_user, gs.embed_item = gu.data_ptr(), gi.data_ptr()
        pi = pj = g = None
        if pred is not None:
            pi, pj, g = (torch.empty(n, device=dev) for _ in range(3))
            pred.update({"prediction_i": pi, "prediction_j": pj, "g": g})
        lib = _capi.load()
        prm = m.bpr_params()
        need = lib.nais_bpr_train_step_workspace_size(prm, n)
        if self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=dev)
        self.step_count += 1
        _capi.check(lib.nais_bpr_train_step(
            prm, user.data_ptr(), item_i.data_ptr(), item_j.data_ptr(), n, uorder.data_ptr(),
            iorder.data_ptr(), self.lr, self.weight_decay, self._st_u.data_ptr(),
            self._st_i.data_ptr(), self.step_count, self.loss_sum.data_ptr(), self._err.data_ptr(),
            _capi.ptr(pi), _capi.ptr(pj), _capi.ptr(g), gs if grads is not None else None,
            self._ws.data_ptr(), self._ws.numel(), _capi.stream_handle(dev)), "nais_bpr_train_step")
        self._bump_versions()

    def _bump_versions(self):
        """As NAISTrainer._bump_versions: the step writes through raw pointers."""
        for q in self.model.parameters():
            increment_version(q)

    def epoch(self, batch_size=4096, shuffle=True):
        """run.py:490-509: the users (shuffled as run.py:490-491) in batches of `batch_size`, one
        batch() and one step() each. Returns the epoch's loss (run.py:507's `lo`), read with the
        epoch's one host sync."""
        users = np.arange(self.csr.shape[0], dtype=np.int64)
        if shuffle:
            users = users[torch.randperm(len(users)).numpy()]
        self.model.train()
        self.loss_sum.zero_()
        for b0 in range(0, len(users), int(batch_size)):
            u, i, j = self.batch(users[b0:b0 + int(batch_size)])
            if u.numel():
                self.step(u, i, j)
        return self.finish()

    def finish(self):
        """Host sync: the accumulated loss. Raises if a step saw an id outside its table or a
        batch could not be drawn (that step and every later one left the tables untouched)."""
        err = int(self._err.item())
        if err:
            self._err.zero_()
            raise RuntimeError(f"BPRTrainer: an id outside its table or an undrawable batch (code {err}); "
                               "that step and the later ones were not applied")
        return float(self.loss_sum.item())


class New1Trainer:
    """train_NAIS_new's loop (run_new.py:391-410) on the device: `batch()` is
    trainDataset.__getitem__ (run_new.py:107-137), `step()` is run_new.py:403-410 (forward,
    loss_func = nn.BCELoss, backward, torch.optim.Adam(lr, betas, eps, weight_decay), which is
    dense: every element of the five tensors moves on every step) updating the model in place,
    `epoch()` the loop with one host sync at its end. Adam's exp_avg / exp_avg_sq live in the
    trainer (`optimizer_state()` / `load_optimizer_state()` exchange them with torch.optim.Adam).
    A step is deterministic: the same batch from the same state gives the same bits.

    The reference cannot train on a user with fewer than 2 history items (its positive row has no
    unmasked item, 0 / 0 is NaN and BCELoss raises): `step()` raises ValueError there and
    `epoch()` skips such users, counting them in `skipped_users`."""

    NAMES = ("embed_target.weight", "embed_region.weight", "attn_Q.weight", "attn_K.weight",
             "attn_V.weight")
    _FIELDS = ("embed_target", "embed_region", "attn_q", "attn_k", "attn_v")

    def __init__(self, model, train_matrix, region_of, lr=0.01, weight_decay=1e-7, num_ng=4,
                 betas=(0.9, 0.999), eps=1e-8):
        from .model import New1
        from .new1 import _region_tensor, visit_rates
        if type(model) is not New1:   # New2 derives from New1: its geo term is not in this step
            raise NotImplementedError(f"New1Trainer: {type(model).__name__} is not New1")
        dev = model._check_device()
        if int(num_ng) < 1:
            raise ValueError(f"New1Trainer: num_ng must be at least 1, got {num_ng}")
        self.model, self.dev = model, dev
        X, r64 = visit_rates(train_matrix)
        self.csr = device_csr(X, dev)
        P = model.embed_target.weight.shape[0]
        if self.csr.shape[1] != P:
            raise ValueError(f"train_matrix has {self.csr.shape[1]} POIs, model has {P}")
        self.region_of = _region_tensor(model, region_of, dev)
        self.rate = torch.from_numpy(np.ascontiguousarray(r64, dtype=np.float64)).to(dev)
        self.num_ng, self.lr, self.weight_decay = int(num_ng), float(lr), float(weight_decay)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.step_count = 0        # Adam's step number t
        self._tag = 0              # one stamp value per call, also for a step that set err
        self.skipped_users = 0
        ps = dict(model.named_parameters())
        self.exp_avg = {k: torch.zeros_like(ps[k]) for k in self.NAMES}
        self.exp_avg_sq = {k: torch.zeros_like(ps[k]) for k in self.NAMES}
        self._st_t = torch.zeros(P, dtype=torch.int32, device=dev)
        self._st_h = torch.zeros(P, dtype=torch.int32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        self._ws = torch.empty(0, dtype=torch.uint8, device=dev)
        self._bufs = {}

    def _check_user(self, uid):
        n = int(self.csr.hist_len[uid])
        P = self.csr.shape[1]
        if n < 1:
            raise ValueError(f"New1: empty history (user {int(uid)})")
        if n * self.num_ng > P - n:
            raise ValueError(f"user {int(uid)}: {n} positives x {self.num_ng} negatives exceed the "
                             f"{P - n} POIs outside the history (trainDataset cannot draw them)")
        return n

    def batch(self, uid, seed=None):
        """trainDataset.__getitem__(uid) (run_new.py:107-137) on the device: (hist [n], target [b],
        labels [b], hist_region [n], target_region [b], visit_rate [n] f32), b = n (1 + num_ng);
        the reference's user_history is hist repeated b times. The history is the CSR row in
        ascending order, the negatives are distinct and uniform over the POIs outside it. The
        buffers are reused by the next call of the same shape."""
        n = self._check_user(uid)
        b = n * (1 + self.num_ng)
        if n not in self._bufs:
            d = self.dev
            self._bufs = {n: (torch.empty(n, dtype=torch.int64, device=d),
                              torch.empty(b, dtype=torch.int64, device=d),
                              torch.empty(b, dtype=torch.float32, device=d),
                              torch.empty(n, dtype=torch.int64, device=d),
                              torch.empty(b, dtype=torch.int64, device=d),
                              torch.empty(n, dtype=torch.float32, device=d))}
        hist, tgt, lab, hreg, treg, vr = self._bufs[n]
        if seed is None:
            seed = int(torch.randint(0, 2**62, (1,)).item())
        _capi.check(_capi.load().nais_new1_make_train_batch(
            self.csr.indptr.data_ptr(), self.csr.indices.data_ptr(), self.rate.data_ptr(),
            self.region_of.data_ptr(), int(uid), n, self.csr.shape[1], self.num_ng, seed,
            hist.data_ptr(), hreg.data_ptr(), vr.data_ptr(), tgt.data_ptr(), treg.data_ptr(),
            lab.data_ptr(), self._err.data_ptr(), _capi.stream_handle(self.dev)),
            "nais_new1_make_train_batch")
        return hist, tgt, lab, hreg, treg, vr

    def _state_struct(self):
        s = _capi.NaisNew1AdamState()
        for name, f in zip(self.NAMES, self._FIELDS):
            setattr(s, "m_" + f, self.exp_avg[name].data_ptr())
            setattr(s, "v_" + f, self.exp_avg_sq[name].data_ptr())
        return s

    def step(self, hist, target, labels, hist_region, target_region, visit_rate, pred=None,
             grads=None):
        """One fused step (run_new.py:403-410) on a batch as batch() returns it, or in the
        reference's own layout: user_history / user_history_region [b, n] with equal rows (row 0
        is taken; the reference repeats one history, run_new.py:111, 132), any input with a
        leading 1 (the DataLoader's batch axis), the visit rate as float64. `pred`: optional [b]
        f32 output (sigmoid(pred)); `grads`: optional dict that receives the five dense gradients
        (before weight decay) under the parameter names."""
        m = self.model
        dev = m._check_device(hist, target, labels, hist_region, target_region, visit_rate)
        if hist.dim() == 3:
            hist = hist.reshape(hist.shape[1:])
        if hist_region.dim() == 3:
            hist_region = hist_region.reshape(hist_region.shape[1:])
        if hist.dim() == 2:
            hist = hist[0] if hist.shape[0] else hist.new_empty(0)
        if hist_region.dim() == 2:
            hist_region = hist_region[0] if hist_region.shape[0] else hist_region.new_empty(0)
        hist = hist.reshape(-1).to(torch.int64).contiguous()
        hreg = hist_region.reshape(-1).to(torch.int64).contiguous()
        target = target.reshape(-1).to(torch.int64).contiguous()
        treg = target_region.reshape(-1).to(torch.int64).contiguous()
        labels = labels.reshape(-1).to(torch.float32).contiguous()
        vr = visit_rate.reshape(-1).to(torch.float32).contiguous()
        b, n = target.numel(), hist.numel()
        if n < 2:
            raise ValueError(f"New1: a history of {n} item(s) cannot be trained on: the reference's "
                             "positive row has no unmasked history item, its prediction is NaN and "
                             "BCELoss raises (all elements of input should be between 0 and 1)")
        if b < 1 or labels.numel() != b or treg.numel() != b or hreg.numel() != n or vr.numel() != n:
            raise ValueError(f"labels / target_region must hold b = {b} rows (b >= 1), hist_region / "
                             f"visit_rate n = {n}; got {labels.numel()}, {treg.numel()}, "
                             f"{hreg.numel()}, {vr.numel()}")
        if pred is not None and (pred.dtype != torch.float32 or pred.numel() != b
                                 or not pred.is_contiguous()):
            raise ValueError("pred must be a contiguous float32 tensor of b elements")
        gs = _capi.NaisNew1TrainGrads()
        if grads is not None:
            ps = dict(m.named_parameters())
            for name, f in zip(self.NAMES, self._FIELDS):
                g = torch.empty_like(ps[name])
                grads[name] = g
                setattr(gs, f, g.data_ptr())
        lib = _capi.load()
        prm = m.new1_params()
        need = lib.nais_new1_train_step_workspace_size(prm, b, n)
        if self._ws.numel() < need:
            self._ws = torch.empty(int(need * 1.25) + 256, dtype=torch.uint8, device=dev)
        self.step_count += 1
        self._tag += 1
        _capi.check(lib.nais_new1_train_step(
            prm, hist.data_ptr(), hreg.data_ptr(), vr.data_ptr(), target.data_ptr(), treg.data_ptr(),
            labels.data_ptr(), b, n, self.lr, self.weight_decay, self.betas[0], self.betas[1],
            self.eps, self.step_count, self._state_struct(), self._st_t.data_ptr(),
            self._st_h.data_ptr(), self._tag, self.loss_sum.data_ptr(), self._err.data_ptr(),
            _capi.ptr(pred), gs if grads is not None else None, self._ws.data_ptr(),
            self._ws.numel(), _capi.stream_handle(dev)), "nais_new1_train_step")
        self._bump_versions()

    def _bump_versions(self):
        """As NAISTrainer._bump_versions: the step writes through raw pointers."""
        for q in self.model.parameters():
            increment_version(q)

    def epoch(self, users=None, shuffle=True):
        """run_new.py:396-410 over `users` (default: every user, shuffled as the DataLoader of
        run_new.py:383 shuffles them). Users with fewer than 2 history items are skipped and
        counted in `skipped_users` (the reference cannot train on them either). Returns train_loss
        (the sum of the per-batch mean losses, run_new.py:408), read with the epoch's one host
        sync."""
        if users is None:
            users = np.arange(self.csr.shape[0])
        users = np.asarray(users, dtype=np.int64)
        if shuffle:
            users = users[torch.randperm(len(users)).numpy()]
        self.model.train()
        self.loss_sum.zero_()
        for u in users.tolist():
            if int(self.csr.hist_len[u]) < 2:
                self.skipped_users += 1
                continue
            self.step(*self.batch(u))
        return self.finish()

    def finish(self):
        """Host sync: the accumulated loss. Raises if a step saw a repeated target or history
        entry, an id outside its table, a history length that disagrees with the CSR or a NaN
        prediction (the reference raises inside BCELoss there); that step and every later one
        left parameters and state untouched."""
        err = int(self._err.item())
        if err:
            self._err.zero_()
            raise RuntimeError("New1Trainer: a batch had a repeated target or history entry, a "
                               "history length that disagrees with the CSR (1), an id outside its "
                               "table (2) or a NaN prediction (4: all elements of input should be "
                               f"between 0 and 1) (code {err}); that step and the later ones were "
                               "not applied")
        return float(self.loss_sum.item())

    def optimizer_state(self):
        """torch.optim.Adam's per-parameter state {name: {'step', 'exp_avg', 'exp_avg_sq'}} (the
        tensors are the trainer's own, not copies)."""
        return {k: {"step": torch.tensor(float(self.step_count)), "exp_avg": self.exp_avg[k],
                    "exp_avg_sq": self.exp_avg_sq[k]} for k in self.NAMES}

    def load_optimizer_state(self, state):
        """The inverse of optimizer_state(): {name: {'step', 'exp_avg', 'exp_avg_sq'}}, e.g. built
        from torch.optim.Adam's state. Every parameter must be present with one common step."""
        steps = {int(float(state[k]["step"])) for k in self.NAMES}
        if len(steps) != 1:
            raise ValueError(f"New1Trainer: the parameters' step counts differ: {sorted(steps)}")
        for k in self.NAMES:
            for key, dst in (("exp_avg", self.exp_avg[k]), ("exp_avg_sq", self.exp_avg_sq[k])):
                src = state[k][key]
                if tuple(src.shape) != tuple(dst.shape):
                    raise ValueError(f"New1Trainer: {k} {key} is {tuple(src.shape)}, "
                                     f"expected {tuple(dst.shape)}")
                dst.copy_(src.to(device=self.dev, dtype=torch.float32))
        self.step_count = steps.pop()
