"""f2_trainer_*: steps on the device against f2_cnn_loss_gradient (bit for bit, which catches a stale layout after the first
step) and against the float64 evaluation of Keras' RMSprop rule; determinism by seed; the exported weights through K4; and
`train_network(engine="hip")` / `cnn train --engine hip` on the toy task of tests/test_training.py."""
import os

import numpy as np
import pytest

import train_referee as tr
from f2cnn_amd import _lib, cli, config
from f2cnn_amd.model import F2CNNModel, load_model
from f2cnn_amd.scripts.CNN import Training
from f2cnn_amd.trainer import Trainer
from test_training import synthetic_windows, write_training_set

pytestmark = pytest.mark.gpu

ROWS, CHANNELS = 13, 40
LR, RHO, EPS, DECAY = 1e-3, 0.9, 1e-7, 0.5       # (a decay that shows in lr_t after one step)


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(21)
    return rng.random((70, ROWS, CHANNELS)).astype(np.float32), rng.integers(0, 2, 70).astype(np.uint8)


def run(ctx, data, seed, order, batch=32):
    t = Trainer(F2CNNModel.glorot(7, ROWS, CHANNELS, zero_bias=False), lr=LR, rho=RHO, eps=EPS, decay=DECAY, drop=tr.DROP, seed=seed, ctx=ctx)
    t.set_data(*data)
    tally = t.steps(order, batch)
    out = t.weights(), t.accumulators(), t.gradient(), tally, t.iterations
    t.close()
    return out


def test_three_steps_against_the_stateless_gradient_and_the_rmsprop_rule(ctx, data):
    """70 windows at batch 32: steps of 32, 32 and 6. After each one the trainer's gradient is f2_cnn_loss_gradient's bit for bit on
    the weights the step started from, and the new accumulators and weights match the float64 evaluation of the RMSprop rule from
    the device's float32 g, a, p: the weights within 1e-6 |update| + 1 ulp(p) (five float32 roundings and the last one); the
    accumulators, whose "update" is their own new value, within 1e-6 a + 1 ulp(a)."""
    x, y = data
    order = np.random.default_rng(4).permutation(70).astype(np.int64)
    seed = 0xABCDEF0123
    t = Trainer(F2CNNModel.glorot(7, ROWS, CHANNELS, zero_bias=False), lr=LR, rho=RHO, eps=EPS, decay=DECAY, drop=tr.DROP, seed=seed, ctx=ctx)
    t.set_data(x, y)
    assert t.iterations == 0 and all(not a.any() for a in t.accumulators().values())
    for it, (s, m) in enumerate(((0, 32), (32, 32), (64, 6))):
        p0, a0 = t.weights(), t.accumulators()
        loss, hits = t.steps(order[s:s + m], 32)
        assert t.iterations == it + 1
        g, p1, a1 = t.gradient(), t.weights(), t.accumulators()
        before = F2CNNModel(p0, ROWS, CHANNELS)
        want, want_loss, want_hits = before.loss_gradient(x, y, index=order[s:s + m], drop=tr.DROP, seed=seed, step=it, ctx=ctx)
        before.release(ctx)
        for k in tr.TENSORS:
            assert g[k].tobytes() == want[k].tobytes(), (it, k)
        assert (loss, hits) == (want_loss, want_hits)
        lr_t = LR / (1.0 + DECAY * it)
        for k in tr.TENSORS:
            gm = g[k].astype(np.float64) / m
            a64 = RHO * a0[k].astype(np.float64) + (1.0 - RHO) * gm * gm
            upd = lr_t * gm / (np.sqrt(a64) + EPS)
            p64 = p0[k].astype(np.float64) - upd
            ea = np.abs(a1[k] - a64) - (1e-6 * a64 + np.spacing(np.abs(a1[k])))
            ep = np.abs(p1[k] - p64) - (1e-6 * np.abs(upd) + np.spacing(np.abs(p0[k])))
            print("step {} {}: accumulator excess {:.3g}, weight excess {:.3g}, max |update| {:.3g}".format(
                it, k, float(ea.max()), float(ep.max()), float(np.abs(upd).max())))
            assert (ea <= 0).all() and (ep <= 0).all(), (it, k)
            assert np.abs(upd).max() > 0
    t.close()


def test_one_step_over_more_than_a_chunk(ctx):
    """batch = 1094: the step's launch works through two chunks of the chain's scratch with the offset device index and masks at
    the places 1024 .. 1093; its gradient and tallies are the stateless call's (which tests/test_gpu_loss_gradient.py holds to the
    referee on these windows)"""
    ref = tr.referee(*tr.CHUNK_CASE, tr.DROP)
    n = len(ref.x)
    seed = 0xABCDEF0123
    order = np.arange(n, dtype=np.int64)
    t = Trainer(ref.model, lr=LR, rho=RHO, eps=EPS, decay=DECAY, drop=tr.DROP, seed=seed, ctx=ctx)
    t.set_data(ref.x, ref.y)
    loss, hits = t.steps(order, n)
    assert t.iterations == 1
    g = t.gradient()
    t.close()
    model = F2CNNModel(ref.model.tensors, ROWS, CHANNELS)         # (a model of this test's own: its device copy lives on this context)
    want, want_loss, want_hits = model.loss_gradient(ref.x, ref.y, drop=tr.DROP, seed=seed, step=0, ctx=ctx)
    indexed, il, ih = model.loss_gradient(ref.x, ref.y, index=order, drop=tr.DROP, seed=seed, step=0, ctx=ctx)
    model.release(ctx)
    for k in tr.TENSORS:
        assert g[k].tobytes() == want[k].tobytes() == indexed[k].tobytes(), k
    assert (loss, hits) == (want_loss, want_hits) == (il, ih)


def test_same_seed_same_bytes(ctx, data):
    order = np.random.default_rng(5).permutation(70).astype(np.int64)
    a = run(ctx, data, 11, order)
    b = run(ctx, data, 11, order)
    c = run(ctx, data, 12, order)
    assert a[4] == b[4] == 3 and a[3] == b[3]
    for k in tr.TENSORS:
        assert a[0][k].tobytes() == b[0][k].tobytes() and a[1][k].tobytes() == b[1][k].tobytes() and a[2][k].tobytes() == b[2][k].tobytes()
    assert any(a[0][k].tobytes() != c[0][k].tobytes() for k in tr.TENSORS)


def test_exported_weights_through_k4(ctx):
    ref = tr.referee(*tr.CASES[0], tr.DROPS[0])
    t = Trainer(ref.model, lr=LR, decay=0.0, drop=tr.DROP, seed=1, ctx=ctx)
    t.set_data(ref.x, ref.y)
    t.steps(np.arange(64, dtype=np.int64), 32)
    model = t.model()
    t.close()
    import torch
    w = tr.torch_weights(model, torch.float64)
    ones = tr.masks_for(np.arange(len(ref.x)), model.rows, model.channels, (0.0, 0.0, 0.0))
    with torch.no_grad():
        _, _, _, p1 = tr._head(w, torch.tensor(ref.x, dtype=torch.float64)[:, None], torch.float64)
        logits = tr._tail(w, p1, ones, torch.float64)[4]
        want = torch.softmax(logits, dim=1).numpy()
    got = model.predict(ref.x, ctx=ctx)
    print("max |K4 - float64 referee| on the trained weights {:.3g}".format(float(np.abs(got - want).max())))
    np.testing.assert_allclose(got, want, atol=2e-5)
    assert any(not np.array_equal(model.tensors[k], ref.model.tensors[k]) for k in tr.TENSORS)


def test_toy_task_trains_through_train_network():
    x, y = synthetic_windows(256, 5)
    xn = Training.normalizeInputBatch(x)
    model, hist = Training.train_network(xn[:192], y[:192], xn[192:], y[192:], batch_size=16, epochs=12, seed=3, verbose=0, engine="hip")
    assert set(hist) == {"loss", "acc", "val_loss", "val_acc"} and len({len(v) for v in hist.values()}) == 1 and len(hist["loss"]) >= 1
    print("hip engine history", hist)
    assert isinstance(model, F2CNNModel) and hist["loss"][-1] < hist["loss"][0]
    _, labels = model.predict_labels(xn[192:])
    assert (labels == y[192:]).mean() >= 0.9
    again, hist2 = Training.train_network(xn[:192], y[:192], xn[192:], y[192:], batch_size=16, epochs=2, seed=3, verbose=0, engine="hip")
    assert hist2["loss"] == hist["loss"][:2]                       # the same seed gives the same run


def test_cnn_train_cli_with_the_hip_engine(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    config.write_default(batch_size=16, epochs=12)
    x, y, split = write_training_set(str(tmp_path), n_train=192, n_test=64)
    assert cli.main(["cnn", "train", "--engine", "hip"]) == 0
    out = capsys.readouterr().out
    assert "Test accuracy:" in out and os.path.isfile("last_trained_model") and os.path.isfile("last_trained_model_results.json")
    model = load_model("last_trained_model")
    xt = Training.normalizeInputBatch(x[split == "TEST"])
    _, labels = model.predict_labels(xt)
    assert (labels == y[split == "TEST"]).mean() >= 0.9
