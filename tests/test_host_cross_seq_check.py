"""tests/cross_seq_check.py proves itself: the float32 model of cross_attn_seq_kernel passes the per-element bound at every edge the
GPU test runs, every deliberate mutation of the model is caught in at least one regime, and the oracle's crossformer equals the
reference-minted fixture tests/golden/crossformer_seq.npz (which the GPU model test uses too)."""
import numpy as np
import pytest
import torch

from oracle import keds_oracle as O
from tests import cross_seq_check as cs
from tests.conftest import golden_path

PAIRS = cs.pairs()


def _case(B, Lq, Lk, H, regime):
    Q, K, V = cs.inputs(B, Lq, Lk, H, regime, seed=Lq * 1000 + Lk)
    return cs.Layout(Q, K, V, B, Lq, Lk, H), cs.reference(Q, K, V, B, Lq, Lk, H)


def test_pairs_cover_the_edges():
    assert {lk for _, lk in PAIRS} == set(cs.LK_EDGES) and {lq for lq, _ in PAIRS} == set(cs.LQ_EDGES)
    for lk in cs.LK_EDGES:
        assert (1, lk) in PAIRS and (17, lk) in PAIRS
    for lq in cs.LQ_EDGES:
        assert (lq, 33) in PAIRS and (lq, 257) in PAIRS


@pytest.mark.parametrize("Lq,Lk", PAIRS)
def test_model_passes_the_bound(Lq, Lk):
    """every (Lq, Lk), (B, heads) and regime of the GPU test"""
    msgs, worst = [], 0.0
    for B, H in cs.BH:
        for regime in cs.REGIMES:
            lay, R = _case(B, Lq, Lk, H, regime)
            obuf = cs.model(lay)
            assert bool((obuf[:, lay.inner:] == cs.SENT).all())
            f, w = cs.failures(lay.out_window(obuf), R, B, Lq, H, f"Lq{Lq}.Lk{Lk}.B{B}.H{H}.{regime}")
            msgs += f
            worst = max(worst, w)
    assert not msgs, "\n".join(msgs)
    assert worst <= 1.0 and (worst > 0.0 or Lk == 1)          # (one key: the output is v itself, exactly)


MUT_SHAPES = ((1, 1), (17, 15), (17, 33), (1, 97), (33, 257), (17, 287))      # (Lq, Lk): every key-tile count, pad keys at each


@pytest.mark.parametrize("mutation", cs.MUTATIONS)
def test_every_mutation_is_caught(mutation):
    """at every shape where the mutation is a defect, some regime fails the bound"""
    ran = 0
    for Lq, Lk in MUT_SHAPES:
        B, H = 3, 2
        if not cs.applicable(mutation, B, Lq, Lk):
            continue
        caught = []
        for regime in cs.REGIMES:
            lay, R = _case(B, Lq, Lk, H, regime)
            f, _ = cs.failures(lay.out_window(cs.model(lay, mutation)), R, B, Lq, H)
            if f:
                caught.append(regime)
        assert caught, f"{mutation} at Lq={Lq}, Lk={Lk} passes the bound in every regime"
        ran += 1
    assert ran >= 3


def test_pad_and_missing_keys_show_in_ramp():
    """the regime built for them: one unmasked zero pad key, or the last key missing, at 287 keys"""
    B, H, Lq, Lk = 3, 2, 17, 287
    lay, R = _case(B, Lq, Lk, H, "ramp")
    for mutation in ("pad", "droplast"):
        f, w = cs.failures(lay.out_window(cs.model(lay, mutation)), R, B, Lq, H)
        assert f and w > 10.0


def test_oracle_crossformer_equals_the_reference_fixture():
    g = dict(np.load(golden_path("crossformer_seq.npz")))
    sd = O.synth_crossformer_state_dict(128, 3, seed=5)
    assert abs(float(sum(v.double().sum().item() for v in sd.values())) - float(g["weights_checksum"])) < 1e-6
    t = {k: torch.from_numpy(v) for k, v in g.items() if v.ndim >= 2}
    cases = (("out_1_77", "q1", "k77", "k77"), ("out_5_77", "q5", "k77", "v77"), ("out_17_257", "q17", "k257", "k257"))
    for name, q, k, v in cases:
        got = O.crossformer(sd, t[q], t[k], t[v])
        assert got.shape == t[name].shape
        assert float((got - t[name]).abs().max()) <= 1e-5, name
    got = O.crossformer(sd, t["late_q"].unsqueeze(1), t["late_k"], t["late_k"])
    assert float((got - t["late_out"]).abs().max()) <= 1e-5
