"""Rare class sampling (RCS), host side (no GPU): the op registration, the C ABI's declarations and argument
checks, the class probabilities, the two-variate draw, the batch sampler behind a DataLoader, the crop selection
rule, the statistics' file round trip and the augment sampler's stream behind RcsCrop.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from adaptsegnet_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rcs_ref as RR  # noqa: E402

SYMS = ("adaptseg_label_class_count", "adaptseg_crop_class_count", "adaptseg_crop_class_count_workspace_size")
OPS = ["label_class_count", "crop_class_count"]


# ---- registration and the C ABI ---------------------------------------------------------------------
def test_ops_are_registered_beside_the_other_lists():
    from adaptsegnet_amd import ops
    assert ops.RCS_NAMES == OPS
    others = (set(ops.NAMES) | set(ops.LOSS_NAMES) | set(ops.MIX_NAMES) | set(ops.MIC_NAMES) | set(ops.AUG_NAMES)
              | set(ops.FDA_NAMES))
    assert not set(OPS) & others       # the other op sets are as they were
    for name in ops.RCS_NAMES:
        op = getattr(torch.ops.adaptseg, name).default
        assert torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CUDA"), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(op.name(), "CPU"), name
        schema = op._schema
        assert len(schema.returns) == 0, name
        assert any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), name
        assert getattr(ops.OPS, name) is op


def test_fake_tensor_tracing():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from adaptsegnet_amd.ops import OPS as O
    with FakeTensorMode():
        lab = torch.empty(2, 40, 68, dtype=torch.uint8, device="cuda")
        cls = torch.empty(2, dtype=torch.int32, device="cuda")
        assert O.label_class_count(lab, None, 19, torch.empty(2, 19, dtype=torch.int64, device="cuda")) is None
        assert O.crop_class_count(lab, None, cls, [32, 16, 0, 0, 0] * 6, 16, 32,
                                  torch.empty(2, 3, dtype=torch.int64, device="cuda")) is None


def test_entry_points_are_declared_and_exported():
    for s in SYMS:
        assert s in _lib.header_symbols(), s
        assert s in _lib._SIGS, s
        assert hasattr(_lib.lib(), s), s
    text = open(_lib.HEADER_PATH).read()
    assert f"#define ADAPTSEG_RCS_MAX_CANDIDATES {_lib.RCS_MAX_CANDIDATES}" in text
    assert _lib.RCS_MAX_CANDIDATES == 16
    assert set(_lib.header_symbols()) == set(_lib._SIGS)


def _params(n, k, row=(48, 32, 0, 0, 0)):
    flat = list(row) * (n * k)
    return (ctypes.c_int32 * len(flat))(*flat)


def test_abi_argument_checks_run_on_the_host():
    L = _lib.lib()
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is rejected before a launch
    err = lambda: L.adaptseg_last_error().decode()  # noqa: E731

    def count(n=2, h=8, w=8, ncls=19, ids=p, counts=p):
        return L.adaptseg_label_class_count(n, h, w, ids, None, ncls, counts, None)

    assert count(n=0) == 1 and "label_class_count" in err()
    assert count(n=65536) == 1 and "65535" in err()
    assert count(h=0) == 1 and count(w=-1) == 1
    assert count(h=1 << 16, w=1 << 15) == 1 and "2^31" in err()
    assert count(ncls=0) == 1 and "num_classes 0" in err()      # a class range outside 1..255
    assert count(ncls=256) == 1 and "num_classes 256" in err()
    assert count(ids=None) == 1 and "null" in err()
    assert count(counts=None) == 1 and "null" in err()

    def crop(n=2, in_h=64, in_w=128, ch=32, cw=48, k=3, params=None, ws=p, ws_bytes=1 << 30, **kw):
        a = dict(ids=p, classes=p, counts=p) | kw
        pa = params if params is not None else _params(n, max(k, 1))
        return L.adaptseg_crop_class_count(n, in_h, in_w, ch, cw, k, a["ids"], None, a["classes"], pa, a["counts"],
                                           ws, ws_bytes, None)

    def size(n=2, in_h=64, in_w=128, ch=32, cw=48, k=3, params=None):
        b = ctypes.c_size_t(0)
        pa = params if params is not None else _params(n, max(k, 1))
        return L.adaptseg_crop_class_count_workspace_size(n, in_h, in_w, ch, cw, k, pa, ctypes.byref(b)), b.value

    for fn in (crop, lambda **kw: size(**kw)[0]):
        assert fn(k=0) == 1 and "crop_class_count" in err() and "K 0" in err()
        assert fn(k=17, params=_params(2, 17)) == 1 and "K 17" in err() and "16" in err()
        assert fn(n=0, params=_params(1, 3)) == 1
        assert fn(n=1, ch=1 << 16, cw=1 << 15, params=_params(1, 3)) == 1 and "2^31" in err()   # ch * cw = 2^31
        assert fn(params=_params(2, 3, (48, 32, 0, 0, 2))) == 1 and "mirror flag 2" in err()
        assert fn(params=_params(2, 3, (48, 32, 0, 0, -1))) == 1 and "mirror" in err()
        assert fn(params=_params(2, 3, (0, 32, 0, 0, 0))) == 1 and "scaled size" in err()
        assert fn(params=_params(2, 3, (1 << 20, 32, 0, 0, 0))) == 1 and "scaled size" in err()
        assert fn(params=_params(2, 3, (48, 32, 1 << 20, 0, 0))) == 1 and "offset" in err()
        assert fn(params=_params(2, 3, (48, 32, 0, -(1 << 20), 0))) == 1 and "offset" in err()
        assert fn(params=_params(2, 3, (4, 32, 0, 0, 0))) == 1 and "downscale" in err()          # 128 -> 4: 32x
    # a bad candidate anywhere in the table is found, and named
    flat = [48, 32, 0, 0, 0] * 6
    flat[5 * 4 + 4] = 7
    assert crop(params=(ctypes.c_int32 * 30)(*flat)) == 1 and "sample 1, candidate 1" in err()
    for name in ("ids", "classes", "counts"):
        assert crop(**{name: None}) == 1 and "null" in err(), name
    st, need = size()
    assert st == 0 and need > 0
    assert crop(ws_bytes=need - 1) == 4 and "workspace" in err()      # ADAPTSEG_ERR_WORKSPACE
    assert crop(ws=None, ws_bytes=need) == 4 and "workspace" in err()


def test_python_surface_validates_before_the_library():
    from adaptsegnet_amd import rcs
    lab = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU"):
        rcs.label_class_count(lab)
    with pytest.raises(ValueError, match="uint8"):
        rcs.label_class_count(lab.float())
    cand = np.tile(np.array([8, 8, 0, 0, 0], np.int32), (2, 3, 1))
    with pytest.raises(ValueError, match="GPU"):
        rcs.crop_class_count(lab, [0, 1], cand, (8, 8))
    with pytest.raises(ValueError, match="tries"):
        rcs.RcsCrop(None, tries=17)
    with pytest.raises(ValueError, match="tries"):
        rcs.RcsCrop(None, tries=0)


# ---- class probabilities ------------------------------------------------------------------------------
def _toy_counts(seed=0, n=40, c=6):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 20000, size=(n, c)).astype(np.int64)
    counts[:, 0] += 200000            # a frequent class
    counts[:, 4] //= 4                # a rare class: at most 4999 pixels, few images above the threshold
    counts[:, 5] = rng.integers(0, 3000, size=n)   # occurs, never above 3000: not eligible
    return counts


def test_class_prob_matches_the_restatement():
    from adaptsegnet_amd import rcs
    counts = _toy_counts()
    for temperature, min_pixels in ((0.01, 3000), (0.1, 100), (1.0, 0)):
        s = rcs.RareClassSampler(rcs.ClassStats(counts), temperature=temperature, min_pixels=min_pixels)
        prob, eligible, images_with = RR.class_prob(counts, temperature, min_pixels)
        np.testing.assert_allclose(s.class_prob, prob, rtol=1e-12, atol=0)
        assert s.class_prob.dtype == np.float64
        assert (s.class_prob[~eligible] == 0).all() and (s.class_prob[eligible] > 0).all()
        assert abs(s.class_prob.sum() - 1.0) < 1e-12
        for a, b in zip(s.images_with, images_with):
            np.testing.assert_array_equal(a, b)
    s = rcs.RareClassSampler(rcs.ClassStats(counts), temperature=0.1)
    assert not s.eligible[5] and s.class_prob[5] == 0          # occurs, but no image with enough of it
    assert counts[:, 4].sum() < counts[:, 0].sum() and s.class_prob[4] > s.class_prob[0]   # rarer: more likely
    assert s.cdf[4] == 1.0                                     # the last eligible entry


def test_eligibility_is_strict_and_none_eligible_raises():
    from adaptsegnet_amd import rcs
    counts = np.array([[5000, 3000, 0], [100, 2999, 0]], np.int64)
    s = rcs.RareClassSampler(rcs.ClassStats(counts), min_pixels=3000)
    assert list(s.eligible) == [True, False, False]            # exactly min_pixels does not make class 1 eligible
    assert s.class_prob[0] == 1.0 and s.class_prob[1] == 0.0
    s = rcs.RareClassSampler(rcs.ClassStats(counts), min_pixels=2999)
    assert list(s.eligible) == [True, True, False] and list(s.images_with[1]) == [0]
    with pytest.raises(ValueError, match="no class"):
        rcs.RareClassSampler(rcs.ClassStats(counts), min_pixels=5000)


# ---- the draw -----------------------------------------------------------------------------------------
def _rng(seed, rank):
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, rank])))


def test_sample_matches_the_restatement_and_draws_two_variates_per_sample():
    from adaptsegnet_amd import rcs
    counts = _toy_counts(3)
    s = rcs.RareClassSampler(rcs.ClassStats(counts), temperature=0.5, seed=11, rank=2)
    prob, eligible, images_with = RR.class_prob(counts, 0.5, 3000)
    ref = _rng(11, 2)
    idx, cls = s.sample(37)
    ridx, rcls = RR.draw(ref, prob, eligible, images_with, 37)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(cls, rcls)
    assert idx.dtype == np.int64 and cls.dtype == np.int64
    assert len(set(cls.tolist())) > 1
    assert (counts[idx, cls] > 3000).all()                    # every image holds enough of its class
    # exactly two variates per sample: a generator advanced by hand is in the same state
    hand = _rng(11, 2)
    for c in cls:
        hand.random()
        hand.integers(len(images_with[c]))
    assert hand.bit_generator.state == s.get_state()
    hand.random()
    assert hand.bit_generator.state != s.get_state()


def test_sample_is_reproducible_per_seed_and_rank_and_resumable():
    from adaptsegnet_amd import rcs
    stats = rcs.ClassStats(_toy_counts(5))
    a = rcs.RareClassSampler(stats, temperature=0.5, seed=4, rank=0)
    b = rcs.RareClassSampler(stats, temperature=0.5, seed=4, rank=0)
    c = rcs.RareClassSampler(stats, temperature=0.5, seed=4, rank=1)
    d = rcs.RareClassSampler(stats, temperature=0.5, seed=5, rank=0)
    ia, ca = a.sample(50)
    ib, cb = b.sample(50)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(ca, cb)
    assert not np.array_equal(ia, c.sample(50)[0]) and not np.array_equal(ia, d.sample(50)[0])
    state = a.get_state()
    nxt = a.sample(20)
    e = rcs.RareClassSampler(stats, temperature=0.5, seed=99, rank=3)
    e.set_state(state)
    res = e.sample(20)
    np.testing.assert_array_equal(nxt[0], res[0])
    np.testing.assert_array_equal(nxt[1], res[1])


class _Toy(torch.utils.data.Dataset):
    def __len__(self):
        return 40

    def __getitem__(self, i):
        return torch.tensor(i)


def test_batch_iter_feeds_a_dataloader_and_pending_pops_in_batch_order():
    from adaptsegnet_amd import rcs
    counts = _toy_counts(7)
    s = rcs.RareClassSampler(rcs.ClassStats(counts), temperature=0.5, seed=21)
    twin = rcs.RareClassSampler(rcs.ClassStats(counts), temperature=0.5, seed=21)
    loader = torch.utils.data.DataLoader(_Toy(), batch_sampler=s.batch_iter(4), num_workers=0)
    it = iter(loader)
    for _ in range(5):
        batch = next(it)
        cls = s.pending.popleft()
        idx, rcls = twin.sample(4)
        np.testing.assert_array_equal(batch.numpy(), idx)
        np.testing.assert_array_equal(cls, rcls)
        assert (counts[batch.numpy(), cls] > 3000).all()


# ---- the selection rule -------------------------------------------------------------------------------
def test_selection_rule_on_hand_written_tables():
    from adaptsegnet_amd import rcs
    table = np.array([[0, 1501, 9000, 10],       # first passing: 1, not the largest
                      [10, 20, 30, 40],          # none passing: the last
                      [1500, 1500, 1500, 1500],  # the threshold is strict: none passes
                      [1500, 1500, 1501, 0],
                      [2000, 0, 0, 0]], np.int64)
    want = [1, 3, 3, 2, 0]
    np.testing.assert_array_equal(rcs.select_crops(table, 1500), want)
    np.testing.assert_array_equal(RR.select(table, 1500), want)
    np.testing.assert_array_equal(rcs.select_crops(np.array([[0], [5000]]), 1500), [0, 0])      # K = 1
    np.testing.assert_array_equal(RR.select(np.array([[0], [5000]]), 1500), [0, 0])
    assert rcs.select_crops(table, 1500).dtype == np.int64
    rng = np.random.default_rng(0)
    t = rng.integers(0, 3000, size=(64, 10))
    np.testing.assert_array_equal(rcs.select_crops(t, 1500), RR.select(t, 1500))


# ---- ClassStats and RcsCrop ---------------------------------------------------------------------------
def test_class_stats_round_trip(tmp_path):
    from adaptsegnet_amd import rcs
    counts = _toy_counts(9)
    path = tmp_path / "stats.npz"
    rcs.ClassStats(counts).save(path)
    back = rcs.ClassStats.load(path)
    np.testing.assert_array_equal(back.counts, counts)
    assert back.counts.dtype == np.int64 and back.num_classes == 6 and len(back) == 40
    with np.load(path, allow_pickle=False) as f:           # arrays only
        assert f.files == ["counts"]
    with pytest.raises(ValueError):
        rcs.ClassStats(np.zeros((3,), np.int64))
    with pytest.raises(ValueError):
        rcs.ClassStats(np.zeros((3, 2), np.float32))


def test_rcs_crop_advances_the_augment_sampler_by_n_times_tries(monkeypatch):
    from adaptsegnet_amd import data, rcs
    seen = {}

    def fake_counts(labels_u8, classes, candidates, crop_size, lut=None):
        seen["cand"] = np.array(candidates)
        k = candidates.shape[1]
        return torch.tensor([[0] * (k - 2) + [2000, 0], [0] * k, [3000] * k], dtype=torch.int64)

    monkeypatch.setattr(rcs, "crop_class_count", fake_counts)
    sampler = data.AugmentSampler((48, 32), seed=5)
    twin = data.AugmentSampler((48, 32), seed=5)
    crop = rcs.RcsCrop(sampler, tries=7, min_crop_pixels=1500)
    labels = torch.zeros(3, 64, 128, dtype=torch.uint8)
    params = crop.params(labels, [1, 2, 3])
    drawn = twin.sample(3 * 7)
    assert sampler.get_state() == twin.get_state()           # exactly n * tries draws
    np.testing.assert_array_equal(seen["cand"], drawn.reshape(3, 7, 5))
    assert params.dtype == np.int32 and params.shape == (3, 5)
    np.testing.assert_array_equal(params, drawn.reshape(3, 7, 5)[[0, 1, 2], [5, 6, 0]])
