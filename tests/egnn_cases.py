"""Inputs of tests/test_egnn_layers_gpu.py (TEST INFRASTRUCTURE): the structures, the weight sets, and the one routine that
runs them through an encoder and collects per-layer node features.  The routine runs in the test process (the default split-bf16
edge GEMM) and, as `python egnn_cases.py OUT.npz`, in a fresh child with MS_EGNN_SPLIT=0 (the fp32 form; the switch is read once
per process), so both forms see the same inputs."""
import os
import sys

import numpy as np

# one partial tile (11^2 = 121 edges), a tile + 16 edges (12^2), exactly 2 and 32 tiles (16^2, 64^2), a last tile with 89 of 128
# edges (91^2) and one 7 short of full (181^2), rows that coincide with the 32-edge units (32, 64, 128) and rows that straddle
# every unit (33, 65, 129); N = 257 has 10 records per residue
LENGTHS = (1, 2, 11, 12, 16, 31, 32, 33, 45, 64, 65, 91, 127, 128, 129, 181, 257)
SET_LENGTHS = (33, 129, 181)
GEOM_LENGTHS = (45, 129)
GEOMETRIES = ("coincident", "two_halves", "far_walk", "extended30")
WEIGHT_SETS = ("seed1", "seed2", "d2scale1", "w2_logspread", "b1_minus8", "gate_plus20", "gate_minus20", "layer1_x4", "layer2_x4")
GEOM_SETS = ("seed0", "d2scale1")


def walk(n, seed=None):
    from merizo_search_amd.foldclass import synthetic as syn
    return syn.random_walk(n, seed=4100 + n if seed is None else seed)


def length_structures():
    return [walk(n) for n in LENGTHS]


def set_structures():
    return [walk(n) for n in SET_LENGTHS]


def geometry(name, n):
    if name == "coincident":                      # d2 = 0 on every edge
        return np.tile(np.array([[1.5, -2.25, 3.0]], dtype=np.float32), (n, 1))
    if name == "two_halves":                      # two coincident halves 7.5 A apart: d2 is 0 or 56.25
        c = np.zeros((n, 3), dtype=np.float32)
        c[n // 2:, 0] = 7.5
        return c
    if name == "far_walk":                        # a walk translated by +1e4 A: coordinates lose 3 decimal digits to the offset
        return (walk(n, seed=4300 + n).astype(np.float64) + 1e4).astype(np.float32)
    if name == "extended30":                      # an extended chain, 30 A per step: d2 up to (30 (n - 1))^2 = 1.5e7 at n = 129
        c = np.zeros((n, 3), dtype=np.float32)
        c[:, 0] = 30.0 * np.arange(n)
        return c
    raise KeyError(name)


def geometry_structures():
    return [geometry(g, n) for g in GEOMETRIES for n in GEOM_LENGTHS]


def weight_set(name):
    """(weights, pe) of a named set: synthetic_state_dict with named tensors edited here."""
    from merizo_search_amd.foldclass import weights as W
    key = W.layer_key
    if name in ("seed0", "seed1", "seed2"):
        sd = W.synthetic_state_dict(int(name[-1]))
    elif name == "d2scale1":
        sd = W.synthetic_state_dict(0, d2_scale=1.0)
    else:
        sd = W.synthetic_state_dict(0)
        rng = np.random.default_rng(99)
        for layer in range(W.N_LAYERS):
            if name == "w2_logspread":
                # magnitudes log-uniform over 2^-16 .. 2^2, random signs: a wide dynamic range inside one dot product, where the
                # split form's dropped mid.lo / lo.lo terms sit closest to the kept ones
                shape = sd[key(layer, "edge_mlp.2.weight")].shape
                mag = np.exp2(rng.uniform(-16.0, 2.0, size=shape))
                sd[key(layer, "edge_mlp.2.weight")] = (mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
            elif name == "b1_minus8":
                # H lives in the SiLU tail: 1e-3 .. 1e-4 of its input
                sd[key(layer, "edge_mlp.0.bias")] = np.full_like(sd[key(layer, "edge_mlp.0.bias")], -8.0)
            elif name in ("gate_plus20", "gate_minus20"):
                sd[key(layer, "edge_gate.0.bias")] = np.full_like(sd[key(layer, "edge_gate.0.bias")], 20.0 if name == "gate_plus20" else -20.0)
            elif name in ("layer1_x4", "layer2_x4"):          # every weight tensor of the first / of the second EGNN layer x 4
                if layer == int(name[5]) - 1:
                    for suffix, _ in W.LAYER_SPEC:
                        if suffix.endswith("weight"):
                            sd[key(layer, suffix)] = sd[key(layer, suffix)] * np.float32(4.0)
            else:
                raise KeyError(name)
    return W.pack_state_dict(sd)


# (e) more than 1024 structures: the plan kernel's blocked scan with per = ceil(nb / 1024) >= 2 structures per thread.  Lengths cycle
# through 1 .. cycle with one N = 129 first, in the middle and last.  Cycle 9 keeps 1024 and 1025 structures under 8192 residues
# (per = 1 / 2, the small-batch proj / node instantiations); 2048 structures need cycle 5 to stay under (per = 2); (2048, 9) and
# (2500, 9) exceed 8192: per = 2 / 3 meet proj<4> / node<16>.
MANY_BATCHES = ((1024, 9), (1025, 9), (2048, 5), (2048, 9), (2500, 9))
LARGE_COUNT = 64           # (f) 64 x 129 = 8256 residues: just over the 8192 threshold of the large-batch instantiations


def many_keys(nb, cycle):
    """(length, seed) per structure of a batch of (e)."""
    keys = [(1 + i % cycle, i % 7) for i in range(nb)]
    for s, pos in enumerate((0, nb // 2, nb - 1)):
        keys[pos] = (129, s)
    return keys


def many_structure(key):
    n, s = key
    return walk(n, seed=5000 + 10 * n + s)


def all_many_keys():
    return sorted({k for nb, cycle in MANY_BATCHES for k in many_keys(nb, cycle)})


def large_structures():
    return [walk(129, seed=6000 + i) for i in range(LARGE_COUNT)]


def split_by(flat, coords_list):
    """[sum N][128] -> list of [N][128], one per structure."""
    out, pos = [], 0
    for c in coords_list:
        out.append(flat[pos:pos + len(c)])
        pos += len(c)
    return out


def embed_layers(enc, coords_list):
    """(embeddings [B][128], node features [2][sum N][128]) of one ragged launch."""
    e = enc.embed(coords_list).cpu().numpy()
    return e, np.stack([enc.node_features(0), enc.node_features(1)])


def collect():
    """Every input of (a) .. (f) through the encoder of THIS process -> {name: array}."""
    from merizo_search_amd import ops
    out = {}
    enc = ops.EgnnEncoder(*weight_set("seed0"), "cuda:0")
    structs = length_structures()
    out["lengths/batch_emb"], out["lengths/batch"] = embed_layers(enc, structs)
    singles = [embed_layers(enc, [c]) for c in structs]
    out["lengths/single_emb"] = np.concatenate([s[0] for s in singles], axis=0)
    out["lengths/single"] = np.concatenate([s[1] for s in singles], axis=1)
    for name in GEOM_SETS:
        e = enc if name == "seed0" else ops.EgnnEncoder(*weight_set(name), "cuda:0")
        _, out["geometry/" + name] = embed_layers(e, geometry_structures())
    for name in WEIGHT_SETS:
        _, out["set/" + name] = embed_layers(ops.EgnnEncoder(*weight_set(name), "cuda:0"), set_structures())
    # (e): every distinct (length, seed) once on its own, in all_many_keys() order, then the batches
    singles = [embed_layers(enc, [many_structure(k)]) for k in all_many_keys()]
    out["many/single_emb"] = np.concatenate([s[0] for s in singles], axis=0)
    out["many/single"] = np.concatenate([s[1] for s in singles], axis=1)
    for nb, cycle in MANY_BATCHES:
        out["many/%d_%d_emb" % (nb, cycle)], out["many/%d_%d" % (nb, cycle)] = embed_layers(enc, [many_structure(k) for k in many_keys(nb, cycle)])
    # (f): one batch over 8192 residues, and the same structures in two batches under it
    large = large_structures()
    out["large/batch_emb"], out["large/batch"] = embed_layers(enc, large)
    halves = [embed_layers(enc, large[:LARGE_COUNT // 2]), embed_layers(enc, large[LARGE_COUNT // 2:])]
    out["large/halves_emb"] = np.concatenate([h[0] for h in halves], axis=0)
    out["large/halves"] = np.concatenate([h[1] for h in halves], axis=1)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    np.savez(sys.argv[1], **collect())
