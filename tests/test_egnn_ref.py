"""CPU checks of the float64 restatement of the encoder (tests/egnn_ref.py) that the per-layer GPU tests compare against.
These prove the restatement, not a kernel: it must reproduce the reference's goldens and the C oracle to fp32 rounding."""
import os

import numpy as np
import pytest

import egnn_cases
import egnn_ref

SANITY_REL = 1e-5          # fp32 rounding of a literal evaluation, with room: measured 2e-7 .. 2e-6 (pooled), up to 2e-6 per layer


def _rel(a, ref64):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref64).max() / np.abs(ref64).max())


@pytest.mark.parametrize("case", ["M0", "3w5h", "AF-Q96HM7-F1-model_v4", "walk1", "walk2", "walk64", "walk257"])
def test_restatement_pools_to_the_reference_goldens(case, synthetic_weights, golden_dir):
    weights, pe = synthetic_weights
    g = np.load(os.path.join(golden_dir, "egnn.npz"))
    layers, pooled = egnn_ref.egnn_layers(weights, pe, g[f"coords_{case}"])
    assert _rel(g[f"emb_{case}"], pooled) <= SANITY_REL
    if case == "M0":           # the one structure whose per-layer node features the reference recorded
        assert _rel(g["layer1_M0"], layers[0]) <= SANITY_REL
        assert _rel(g["layer2_M0"], layers[1]) <= SANITY_REL


@pytest.mark.slow
def test_restatement_pools_to_the_reference_golden_of_the_longest_chain(synthetic_weights, golden_dir):
    weights, pe = synthetic_weights
    g = np.load(os.path.join(golden_dir, "egnn.npz"))
    case = "AF-Q96PD2-F1-model_v4"          # 775 residues
    assert _rel(g[f"emb_{case}"], egnn_ref.egnn_layers(weights, pe, g[f"coords_{case}"])[1]) <= SANITY_REL


@pytest.mark.parametrize("case", ["M0", "walk97", "walk292"])
def test_restatement_pools_to_the_reference_goldens_at_full_distance_scale(case, golden_dir):
    """d2_scale = 1: pre-activations of +-1e2 .. 1e3, where a naive exp(-x) overflows (the restatement's SiLU must not warn)."""
    from merizo_search_amd.foldclass import weights as W
    g = np.load(os.path.join(golden_dir, "egnn_d2.npz"))
    weights, pe = W.pack_state_dict(W.synthetic_state_dict(0, d2_scale=float(g["d2_scale"])))
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        egnn_ref.silu(np.array([-1e4, -800.0, 0.0, 800.0, 1e4]))
    _, pooled = egnn_ref.egnn_layers(weights, pe, g[f"coords_{case}"])
    assert _rel(g[f"emb_{case}"], pooled) <= SANITY_REL


@pytest.mark.parametrize("name", ["seed0", "d2scale1"])
def test_restatement_layers_agree_with_the_oracle_and_the_distance_helper(name):
    """Per layer and per residue against oracle.egnn_embed(..., return_layers=True), through the helper the GPU tests take
    their bar from: G (relative to the layer's largest value) stays at fp32 rounding; P (relative to the residue's own) is
    reported by the same helper and is never below G."""
    weights, pe = egnn_cases.weight_set(name)
    coords = [egnn_cases.walk(n) for n in (1, 2, 33, 45, 129)] + [egnn_cases.geometry("coincident", 45)]
    refs = [egnn_ref.egnn_layers(weights, pe, c)[0] for c in coords]
    g_orc, p_orc, layers = egnn_ref.oracle_distances(weights, pe, coords, refs)
    print("oracle vs float64 restatement, %s: G %s  P %s" % (name, g_orc, p_orc))
    assert layers.shape == (2, sum(len(c) for c in coords), 128)
    assert (g_orc > 0).all() and (g_orc <= SANITY_REL).all()
    assert (p_orc >= g_orc).all() and (p_orc <= 10 * SANITY_REL).all()


def test_distance_helper_sees_one_lost_message_on_one_residue():
    """What the pooled comparison dilutes: a fault on ONE residue of N moves G and P by its full size."""
    rng = np.random.default_rng(3)
    h64 = rng.standard_normal((257, 128))
    h = h64.astype(np.float32).copy()
    h[100, 7] += np.float32(1e-3)
    g, p = egnn_ref.distances(h, h64)
    assert g == pytest.approx(1e-3 / np.abs(h64).max(), rel=1e-3)
    assert p == pytest.approx(1e-3 / np.abs(h64[100]).max(), rel=1e-3)
    pooled_shift = abs(h.astype(np.float64).mean(axis=0)[7] - h64.mean(axis=0)[7])
    assert pooled_shift < 1e-3 / 200


def test_weight_sets_differ_from_seed0_only_in_the_named_tensors():
    from merizo_search_amd.foldclass import weights as W
    base = W.unpack_weights(egnn_cases.weight_set("seed0")[0])
    touched = {"w2_logspread": "edge_mlp.2.weight", "b1_minus8": "edge_mlp.0.bias", "gate_plus20": "edge_gate.0.bias",
               "gate_minus20": "edge_gate.0.bias"}
    for name, suffix in touched.items():
        sd = W.unpack_weights(egnn_cases.weight_set(name)[0])
        for k in base:
            assert np.array_equal(sd[k], base[k]) == (not k.endswith(suffix)), (name, k)
    w2 = np.abs(W.unpack_weights(egnn_cases.weight_set("w2_logspread")[0])[W.layer_key(0, "edge_mlp.2.weight")])
    assert w2.min() >= 2.0 ** -16 * (1 - 1e-6) and w2.max() <= 4.0 and np.log2(w2).std() > 4.5     # uniform over 18 octaves: std 5.2
    for name, prefix in (("layer1_x4", "encode_ca_egnn.0."), ("layer2_x4", "encode_ca_egnn.1.")):
        sd = W.unpack_weights(egnn_cases.weight_set(name)[0])
        for k in base:
            scaled = k.startswith(prefix) and k.endswith("weight")
            assert np.array_equal(sd[k], base[k] * np.float32(4.0 if scaled else 1.0)), (name, k)
