"""PG_PREC_F16X2 / PG_PREC_F16 restated in numpy — the specification the GPU tests of the fp16 rank modes lean on.

The restatement follows pairec_amd/csrc/rank_2r.hip and the load-time scaling in rank_model.hpp (build_f16_operands, which
tests/test_rank_model_cpu.py runs on the host):
  E_k = floor(log2 max_j |W1[k][j]|) per item input column, F_i = floor(log2 max_j |W2[i][j]|) per hidden unit (0 for a zero row)
  x'_k = fp16(x_k * 2^(E_k + G))          against  W1[k][:] * 2^(-E_k - G + S)   (accumulators: 2^S * z1, c1 enters * 2^S)
  h'_i = fp16(relu(acc1_i) * 2^(F_i + G - S))  against  W2[i][:] * 2^(-F_i - G + S)   (accumulators: 2^S * z2)
  G = 11, S = 23; weights as hi + lo fp16 (F16X2) or one fp16 (F16); layer 3 and the sigmoid in fp32's formula.
fp16 conversion is RNE with everything under 2^-14 FLUSHED to zero (the pessimistic reading of the matrix pipe: the kernel
must not depend on subnormal operands surviving), accumulation is fp64 (the GPU's fp32 accumulation order is not modelled —
the GPU test allows a factor of 2 for it).

Bar: |score - o.dnn3_forward(w, 0, ...)| <= 1e-5 (BASELINE.json north_star), on 4 requests x 5 000 candidates of a 40 000-row
synthetic table at the five DNN3 shapes and on the wide-range construction of tests/test_gpu_bf16x3.py.
Underflow bound: a scaled activation under 2^-14 is below 2^(-14 - G) = 2^-25 in row-normalised units, the normalised weight
below 2, so a flushed term costs less than 2^-24 and a pre-activation at most fan_in * 2^-24 — asserted on a table whose
every column underflows.

Emulated error (the worst value printed per mode over the five shapes and the wide-range case; DESIGN.md §4.2 quotes it):
EMULATED below.  test_the_recorded_emulated_error_is_current holds the constants to what this file computes."""
import numpy as np
import pytest

from oracle import oracle as o

SHAPES = [(128, 128), (256, 128), (256, 256), (512, 256), (1024, 512)]
TOL = 1e-5
G, S = 11, 23
# worst |score - fp32 oracle| of the emulation, per mode (nprod 2 = F16X2, 1 = F16), rounded up to two digits
EMULATED = {2: 3.0e-6, 1: 3.7e-6}


def _floor_log2_rowmax(w):
    mx = np.max(np.abs(w), axis=1)
    e = np.frexp(mx)[1] - 1
    return np.where(mx > 0, e, 0).astype(np.int64)


def _fp16_flushed(a):
    """RNE to fp16 (overflow → inf), results under the smallest normal 2^-14 flushed to zero; returned as fp64."""
    with np.errstate(over="ignore"):
        h = np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float64)
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def _weights(ws, nprod):
    hi = _fp16_flushed(ws)
    if nprod == 1:
        return hi
    return hi + _fp16_flushed((ws.astype(np.float64) - hi).astype(np.float32))


def f16_layer1(w, nprod, user, rows):
    """(z1 as the mode computes it [n][h1] fp64, x' [n][128]) — pre-activations in the model's own units."""
    du = w.d_user
    w1i = w.w1[du:].astype(np.float32)
    E = _floor_log2_rowmax(w1i)
    xs = np.exp2(E + G).astype(np.float32)
    w1s = (w1i * np.exp2(-E - G + S).astype(np.float32)[:, None]).astype(np.float32)      # exact: powers of two
    c1 = (w.b1.astype(np.float64) + user.astype(np.float64) @ w.w1[:du].astype(np.float64)).astype(np.float32)
    xp = _fp16_flushed(rows.astype(np.float32) * xs[None, :])
    acc1 = c1.astype(np.float64)[None, :] * 2.0 ** S + xp @ _weights(w1s, nprod)
    return acc1 * 2.0 ** -S, xp


def f16_forward(w, nprod, user, rows):
    z1, _ = f16_layer1(w, nprod, user, rows)
    F = _floor_log2_rowmax(w.w2)
    hs = np.exp2(F + G - S).astype(np.float32)
    w2s = (w.w2 * np.exp2(-F - G + S).astype(np.float32)[:, None]).astype(np.float32)
    acc1 = (z1 * 2.0 ** S).astype(np.float32)                                              # the fp32 accumulator
    hp = _fp16_flushed(np.maximum(acc1, 0.0) * hs[None, :])
    acc2 = w.b2.astype(np.float64)[None, :] * 2.0 ** S + hp @ _weights(w2s, nprod)
    z3 = w.b3 + np.maximum(acc2, 0.0) @ (w.w3.astype(np.float64) * 2.0 ** -S)
    return 1.0 / (1.0 + np.exp(-z3))


def _requests(n, seed, sizes):
    rng = np.random.default_rng(seed)
    users = o.synth_rows(o.SEED_QUERY, 3, len(sizes), 128)
    cands = [rng.integers(0, n, s_).astype(np.uint32) for s_ in sizes]
    return users, cands


def _worst(w, tab, users, cands):
    worst = {}
    for nprod in (2, 1):
        err = 0.0
        for r in range(len(cands)):
            ref = o.dnn3_forward(w, 0, users[r], tab[cands[r]]).astype(np.float64)
            err = max(err, float(np.max(np.abs(f16_forward(w, nprod, users[r], tab[cands[r]]) - ref))))
        worst[nprod] = err
    return worst


@pytest.fixture(scope="module")
def table():
    return o.synth_rows(o.SEED_TABLE, 0, 40_000, 128)


@pytest.fixture(scope="module")
def errors(table):
    """worst emulated error per (case, mode): the five shapes and the wide-range construction, computed once"""
    out = {}
    for h1, h2 in SHAPES:
        users, cands = _requests(40_000, h1 + h2, [5000] * 4)
        w = o.Dnn3Weights(128, 128, h1, h2, seed=o.SEED_WEIGHTS ^ (h1 + h2))
        out["%d-%d" % (h1, h2)] = _worst(w, table, users, cands)
    # tests/test_gpu_bf16x3.py::test_dnn3_bf16x3_on_inputs_of_a_wide_dynamic_range
    n = 20_000
    scale = np.exp2(np.random.default_rng(11).integers(-20, 13, 128)).astype(np.float32)
    tab_s = (table[:n] * scale[None, :]).astype(np.float32)
    w = o.Dnn3Weights()
    w1 = w.w1.copy()
    w1[128:] = (w1[128:] / scale[:, None]).astype(np.float32)
    w.w1 = w1
    users, cands = _requests(n, 5, [3000, 500])
    out["wide"] = _worst(w, tab_s, users[:2], cands)
    for k_, v in out.items():
        print("emulated %s: f16x2 %.3g  f16 %.3g" % (k_, v[2], v[1]))
    return out


@pytest.mark.parametrize("case", ["%d-%d" % s_ for s_ in SHAPES] + ["wide"])
def test_emulated_fp16_modes_are_within_north_star_of_the_fp32_oracle(errors, case):
    for nprod in (2, 1):
        assert errors[case][nprod] <= TOL, (case, nprod, errors[case][nprod])


def test_the_recorded_emulated_error_is_current(errors):
    for nprod in (2, 1):
        worst = max(v[nprod] for v in errors.values())
        print("emulated error, nprod %d: %.3g (recorded %.3g)" % (nprod, worst, EMULATED[nprod]))
        assert 0.8 * EMULATED[nprod] <= worst <= EMULATED[nprod]


def test_underflow_costs_at_most_fan_in_times_2_to_the_minus_24():
    """Every column of the table just under what survives the fp16 convert: all 128 terms of a pre-activation are lost,
    and the loss stays inside fan_in * 2^-24 — absolutely, in the model's own units."""
    w = o.Dnn3Weights()
    E = _floor_log2_rowmax(w.w1[128:])
    rng = np.random.default_rng(3)
    sign = rng.choice([-1.0, 1.0], (500, 128))
    rows = (sign * (0.999 * np.exp2(-E - G - 14.0))[None, :]).astype(np.float32)
    user = o.synth_rows(o.SEED_QUERY, 3, 1, 128)[0]
    exact = (w.b1.astype(np.float64) + user.astype(np.float64) @ w.w1[:128].astype(np.float64)).astype(np.float32).astype(np.float64)[None, :] \
        + rows.astype(np.float64) @ w.w1[128:].astype(np.float64)
    for nprod in (2, 1):
        z1, xp = f16_layer1(w, nprod, user, rows)
        assert not xp.any()                                     # everything was flushed
        loss = float(np.max(np.abs(z1 - exact)))
        print("nprod %d: all-underflow loss %.3g of the bound %.3g" % (nprod, loss, 128 * 2.0 ** -24))
        assert 0 < loss <= 128 * 2.0 ** -24
    # and one octave up nothing is flushed
    _, xp = f16_layer1(w, 2, user, rows * 2.0)
    assert xp.all()


def test_out_of_range_activations_become_infinite_not_wrong():
    """What the kernel's range flag looks for: a scaled activation past fp16's largest finite value converts to inf."""
    w = o.Dnn3Weights()
    rows = np.zeros((1, 128), np.float32)
    rows[0, 7] = 1e9
    _, xp = f16_layer1(w, 2, o.synth_rows(o.SEED_QUERY, 3, 1, 128)[0], rows)
    assert np.isinf(xp[0, 7])
