"""The HIP encoder per residue and per layer against a float64 restatement (tests/egnn_ref.py), in both edge-GEMM forms.

The pooled 128-vector that tests/test_egnn_gpu.py compares dilutes a fault on one residue of N by 1/N (a lost message: 1/N^2), so
these tests read the node features of both layers back (EgnnEncoder.node_features) and compare every residue.

THE BAR.  For a structure and a layer, G = max |h - h64| / max |h64| over the structure and P = max over residues i of
max_c |h_ic - h64_ic| / max_c |h64_ic| (egnn_ref.distances).  The same two figures are computed for the C oracle -- the
reference's arithmetic as a literal fp32 evaluation, on the CPU, same inputs, same weights -- and their maxima over the structures
of the test's weight set are G_orc and P_orc, per layer.  The kernel must satisfy G <= 4 G_orc and P <= 4 P_orc for every
structure: two fp32 evaluations that differ only in summation order and in a 1-ulp exp / rcp may differ by a couple of bits in
their worst element, and the factor 4 allows two bits.  Nothing here is tuned to what the kernel gives.

Inputs: tests/egnn_cases.py.  The default (split-bf16) form runs in this process; the fp32 form (MS_EGNN_SPLIT=0, read once per
process) in ONE fresh child that dumps every node feature to an .npz.  Both forms meet the same bar."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import egnn_cases as cases
import egnn_ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = ("split", "fp32")
FACTOR = 4.0
MS_ERR_ARG = -1            # include/merizo_search_amd.h


@pytest.fixture(scope="module")
def features(tmp_path_factory):
    """form -> {name: node features / embeddings} of every input, computed once per form."""
    cache = {}

    def get(form):
        if form not in cache:
            if form == "split":
                assert os.environ.get("MS_EGNN_SPLIT", "1") != "0", "this process must run the default form"
                cache[form] = cases.collect()
            else:
                out = str(tmp_path_factory.mktemp("egnn_fp32") / "fp32.npz")
                r = subprocess.run([sys.executable, os.path.join(HERE, "egnn_cases.py"), out], env=dict(os.environ, MS_EGNN_SPLIT="0"),
                                   capture_output=True, text=True, timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                with np.load(out) as z:
                    cache[form] = {k: z[k] for k in z.files}
        return cache[form]
    return get


@functools.lru_cache(maxsize=None)
def reference(group):
    """(coords list, float64 layers per structure, G_orc[2], P_orc[2]) of a group of inputs; computed once, shared by both forms."""
    kind, _, name = group.partition("/")
    if kind == "lengths":
        wset, coords = "seed0", cases.length_structures()
    elif kind == "geometry":
        wset, coords = name, cases.geometry_structures()
    elif kind == "set":
        wset, coords = name, cases.set_structures()
    elif kind == "many129":
        wset, coords = "seed0", [cases.many_structure((129, s)) for s in range(3)]
    else:
        raise KeyError(group)
    weights, pe = cases.weight_set(wset)
    refs = [egnn_ref.egnn_layers(weights, pe, c)[0] for c in coords]
    g_orc, p_orc, _ = egnn_ref.oracle_distances(weights, pe, coords, refs)
    print("\n[bar] %-22s G_orc %.2e %.2e  P_orc %.2e %.2e" % (group, g_orc[0], g_orc[1], p_orc[0], p_orc[1]))
    return coords, refs, g_orc, p_orc


def check_against_float64(group, form, layers, labels=None):
    """layers [2][sum N][128] of the group's structures in order: every structure and layer within FACTOR x the oracle's distance."""
    coords, refs, g_orc, p_orc = reference(group)
    assert layers.shape == (2, sum(len(c) for c in coords), 128) and np.isfinite(layers).all()
    bad, worst = [], np.zeros((2, 2))
    for layer in range(2):
        for s, (h, ref) in enumerate(zip(cases.split_by(layers[layer], coords), refs)):
            g, p = egnn_ref.distances(h, ref[layer])
            worst[layer] = np.maximum(worst[layer], (g, p))
            label = labels[s] if labels else "N=%d" % len(coords[s])
            print("[%s %s] %-16s layer %d  G %.2e (bar %.2e)  P %.2e (bar %.2e)" % (form, group, label, layer, g, FACTOR * g_orc[layer],
                                                                                      p, FACTOR * p_orc[layer]))
            if not (g <= FACTOR * g_orc[layer] and p <= FACTOR * p_orc[layer]):
                bad.append((label, layer, g, p))
    print("[worst %s %s] G %.2e %.2e  P %.2e %.2e | G_orc %.2e %.2e  P_orc %.2e %.2e" % (
        form, group, worst[0, 0], worst[1, 0], worst[0, 1], worst[1, 1], g_orc[0], g_orc[1], p_orc[0], p_orc[1]))
    assert not bad, bad


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---------------------------------------------------------------- (a) per residue, per layer, at every boundary
@pytest.mark.parametrize("form", FORMS)
def test_every_boundary_length_per_residue_and_layer(form, features):
    """One partial tile .. 10 records per residue (egnn_cases.LENGTHS), as one ragged batch and each on its own: the two
    bit-identical, node features and embeddings, and both layers of every structure within the bar."""
    f = features(form)
    assert same_bits(f["lengths/batch"], f["lengths/single"])
    assert same_bits(f["lengths/batch_emb"], f["lengths/single_emb"])
    check_against_float64("lengths", form, f["lengths/batch"])


# ---------------------------------------------------------------- (b) geometry edges
@pytest.mark.parametrize("wset", cases.GEOM_SETS)
@pytest.mark.parametrize("form", FORMS)
def test_geometry_edges_per_residue_and_layer(form, wset, features):
    """All residues coincident (d2 = 0 on every edge), two coincident halves, a walk translated by 1e4 A, an extended chain with
    30 A steps (d2 up to 1.5e7: at d2_scale = 1 the first SiLU saturates on every edge but the diagonal), at N = 45 and 129."""
    labels = ["%s N=%d" % (g, n) for g in cases.GEOMETRIES for n in cases.GEOM_LENGTHS]
    check_against_float64("geometry/" + wset, form, features(form)["geometry/" + wset], labels)


# ---------------------------------------------------------------- (c) weight sets beyond seed 0
@pytest.mark.parametrize("wset", cases.WEIGHT_SETS)
@pytest.mark.parametrize("form", FORMS)
def test_weight_sets_per_residue_and_layer(form, wset, features):
    """Other seeds, the distance column at full scale, edge_mlp.2.weight spread over 18 octaves, H in the SiLU tail, a saturated
    gate either way, the first / the second layer's weights x 4 (egnn_cases.weight_set), on N = 33, 129, 181."""
    check_against_float64("set/" + wset, form, features(form)["set/" + wset])


# ---------------------------------------------------------------- (e) more than 1024 structures
@pytest.mark.parametrize("nb,cycle", cases.MANY_BATCHES)
@pytest.mark.parametrize("form", FORMS)
def test_more_structures_than_plan_threads(form, nb, cycle, features):
    """The plan kernel's blocked scan with 1, 2 and 3 structures per thread, find_segment over more than 1024 segments, and
    tile_pre[nb] / rec_pre[nb]: node features of both layers and the embeddings bit-identical to the same structures embedded
    one by one (by lookup: each distinct (length, seed) was embedded once); the three N = 129 structures -- first, middle, last
    -- within the float64 bar as well."""
    f = features(form)
    keys = cases.many_keys(nb, cycle)
    total = sum(k[0] for k in keys)
    assert (total > 8192) == ((nb, cycle) in ((2048, 9), (2500, 9))), total     # which proj / node instantiations this batch meets
    assert (nb + 1023) // 1024 == {1024: 1, 1025: 2, 2048: 2, 2500: 3}[nb]
    single_keys = cases.all_many_keys()
    starts = np.concatenate([[0], np.cumsum([k[0] for k in single_keys])])
    index = {k: i for i, k in enumerate(single_keys)}
    rows = np.concatenate([np.arange(starts[index[k]], starts[index[k]] + k[0]) for k in keys])
    batch = f["many/%d_%d" % (nb, cycle)]
    assert batch.shape == (2, total, 128)
    expect = f["many/single"][:, rows]
    differing = np.flatnonzero((batch.view(np.uint32) != expect.view(np.uint32)).any(axis=(0, 2)))
    assert differing.size == 0, "first differing residue rows of the batch: %s" % differing[:8]
    assert same_bits(f["many/%d_%d_emb" % (nb, cycle)], f["many/single_emb"][[index[k] for k in keys]])
    offs = np.concatenate([[0], np.cumsum([k[0] for k in keys])])
    long_rows = np.concatenate([np.arange(offs[p], offs[p + 1]) for p in (0, nb // 2, nb - 1)])
    assert [keys[p] for p in (0, nb // 2, nb - 1)] == [(129, 0), (129, 1), (129, 2)]
    check_against_float64("many129", form, batch[:, long_rows], ["first", "middle", "last"])


# ---------------------------------------------------------------- (f) large-batch instantiations per node
@pytest.mark.parametrize("form", FORMS)
def test_large_batch_instantiations_give_the_same_node_features(form, features):
    """64 x 129 = 8256 residues run proj<4> / node<16>; the same structures in two batches of 4128 run proj<1> / node<4>.  'Per
    output the k order of the fmaf chain is the same in every configuration': both layers bit-identical, per node."""
    f = features(form)
    assert f["large/batch"].shape[1] == 64 * 129 > 8192
    assert same_bits(f["large/batch"], f["large/halves"])
    assert same_bits(f["large/batch_emb"], f["large/halves_emb"])


# ---------------------------------------------------------------- (g) the pool kernel alone
def _pool_check(emb, h, coords):
    """The returned embedding = the mean of the GPU's own layer-2 node features, summed exactly (math.fsum) and divided in
    float64, rounded to fp32 -- within 1 fp32 ulp: the kernel sums and divides in float64 and rounds once."""
    for s, hs in enumerate(cases.split_by(h, coords)):
        exact = np.array([math.fsum(col) for col in hs.astype(np.float64).T]) / hs.shape[0]
        ref = exact.astype(np.float32)
        ulps = np.abs(emb[s].astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
        assert ulps.max() <= 1.0, (s, hs.shape[0], ulps.max())


def test_pool_is_the_mean_of_the_layer2_node_features(features):
    f = features("split")
    _pool_check(f["lengths/batch_emb"], f["lengths/batch"][1], cases.length_structures())


@pytest.mark.parametrize("n", [2000, 3000])
def test_pool_of_a_long_chain_is_the_mean_of_its_node_features(n, synthetic_weights):
    from merizo_search_amd import ops
    enc = ops.EgnnEncoder(*synthetic_weights, "cuda:0")
    coords = [cases.walk(n)]
    emb = enc.embed(coords).cpu().numpy()
    h = enc.node_features(1)
    assert h.shape == (n, 128) and np.isfinite(h).all()
    _pool_check(emb, h, coords)


# ---------------------------------------------------------------- the read-out itself
def test_node_features_readout_refuses_bad_arguments(synthetic_weights):
    import ctypes
    from merizo_search_amd import _lib, ops
    enc = ops.EgnnEncoder(*synthetic_weights, "cuda:0")
    with pytest.raises(_lib.MerizoHipError):
        enc.node_features(0)                       # no embed yet
    enc.embed([cases.walk(12), cases.walk(5)])
    with pytest.raises(_lib.MerizoHipError):
        enc.node_features(2)
    lib = _lib.load()
    buf = np.empty((17, 128), dtype=np.float32)
    ws = ctypes.c_void_p(enc._ws.data_ptr())
    good = (2, 17, 169, 0)
    assert lib.ms_debug_egnn_node_features(ws, *good, buf.ctypes.data) == 0
    for nb, total, sum_sq, layer in ((0, 17, 169, 0), (2, 1, 169, 0), (2, 17, 16, 0), (2, 17, 290, 0), (2, 17, 169, -1)):
        assert lib.ms_debug_egnn_node_features(ws, nb, total, sum_sq, layer, buf.ctypes.data) == MS_ERR_ARG
    assert lib.ms_debug_egnn_node_features(None, *good, buf.ctypes.data) == MS_ERR_ARG
    assert lib.ms_debug_egnn_node_features(ws, *good, None) == MS_ERR_ARG
    assert same_bits(buf, enc.node_features(0))
