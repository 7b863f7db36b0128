"""Float64 restatement of the Foldclass encoder in numpy (TEST INFRASTRUCTURE; the product never imports it).

Written from the arithmetic csrc/ms_egnn.hip's header documents, not from its kernels:
    node features h = pe[:N]
    two layers of   z_ij = W1 . [h_i, h_j, d2_ij] + b1        (= W1a.h_i + b1 + W1b.h_j + w_c d2_ij)
                    m_ij = SiLU(W2 . SiLU(z_ij) + b2)
                    g_ij = sigmoid(w_g . m_ij + b_g)
                    m_i  = sum over all j (j == i included) of g_ij m_ij
                    h_i' = Wn2 . SiLU(Wn1 . [h_i, m_i] + bn1) + bn2 + h_i
    embedding = mean over residues of the second layer's h

One input rule: d2 is an INPUT of the comparison, not part of it.  It is formed in float32 by the reference's op sequence
(difference, squares summed, sqrt, then dist * dist) and then widened; everything else is float64.  A row of edges (i fixed,
all j) is processed at a time, so memory stays at N x 514 doubles.

The distances G and P below are what the GPU tests bound (tests/test_egnn_layers_gpu.py) and what the C oracle -- a literal
fp32 evaluation -- is measured by to set that bound.
"""
import numpy as np

DIM, M_DIM, EDGE_IN, EDGE_HID, NODE_IN, NODE_HID = 128, 256, 257, 514, 384, 256
_SHAPES = ((EDGE_HID, EDGE_IN), (EDGE_HID,), (M_DIM, EDGE_HID), (M_DIM,), (1, M_DIM), (1,),
           (NODE_HID, NODE_IN), (NODE_HID,), (DIM, NODE_HID), (DIM,))     # one layer of the blob, state_dict order
LAYER_FLOATS = sum(int(np.prod(s)) for s in _SHAPES)


def sigmoid(x):
    """1 / (1 + exp(-x)) without overflow: exp only ever sees a non-positive argument."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0, e) / (1.0 + e)


def silu(x):
    return x * sigmoid(x)


def _layer_tensors(weights, layer):
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    assert w.size == 2 * LAYER_FLOATS
    out, off = [], layer * LAYER_FLOATS
    for shape in _SHAPES:
        n = int(np.prod(shape))
        out.append(w[off:off + n].reshape(shape).astype(np.float64))
        off += n
    return out


def d2_row(coords32, i):
    """Squared distances of residue i to every residue: float32 by the reference's op sequence, widened."""
    diff = coords32[i][None, :] - coords32                       # float32
    sq = diff * diff
    dist = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    return (dist * dist).astype(np.float64)


def _layer(tensors, h, coords32):
    w1, b1, w2, b2, wg, bg, wn1, bn1, wn2, bn2 = tensors
    n = h.shape[0]
    a = h @ w1[:, :DIM].T + b1                                   # [N,514]: the h_i part of the first edge Linear, with the bias
    b = h @ w1[:, DIM:2 * DIM].T                                 # the h_j part
    wc = w1[:, 2 * DIM]                                          # the distance column
    w2t, wgv = np.ascontiguousarray(w2.T), wg.reshape(-1)
    out = np.empty_like(h)
    for i in range(n):
        z = a[i][None, :] + b + d2_row(coords32, i)[:, None] * wc[None, :]
        m = silu(silu(z) @ w2t + b2)                             # [N,256]
        g = sigmoid(m @ wgv + bg[0])                             # [N]
        mi = (m * g[:, None]).sum(axis=0)
        x = np.concatenate([h[i], mi])
        out[i] = wn2 @ silu(wn1 @ x + bn1) + bn2 + h[i]
    return out


def egnn_layers(weights, pe, coords):
    """One structure -> (node features float64 [2][N][128], pooled embedding float64 [128])."""
    coords32 = np.ascontiguousarray(np.asarray(coords, dtype=np.float32).reshape(-1, 3))
    n = coords32.shape[0]
    h = np.asarray(pe, dtype=np.float32).reshape(-1, DIM)[:n].astype(np.float64)
    layers = np.empty((2, n, DIM), dtype=np.float64)
    for layer in range(2):
        h = _layer(_layer_tensors(weights, layer), h, coords32)
        layers[layer] = h
    return layers, layers[1].mean(axis=0)


def distances(h, h64):
    """(G, P) of one structure and one layer, h and h64 [N][128]:
    G = max |h - h64| / max |h64| over the structure; P = max over residues i of max_c |h_ic - h64_ic| / max_c |h64_ic|."""
    d = np.abs(np.asarray(h, dtype=np.float64) - h64)
    a = np.abs(h64)
    return float(d.max() / a.max()), float((d.max(axis=1) / a.max(axis=1)).max())


def oracle_distances(weights, pe, coords_list, refs):
    """The C oracle's own distance from the restatement: (G_orc[2], P_orc[2], layers), the per-layer maxima of G and P over the
    structures of coords_list; refs[s] is egnn_layers(...)[0] of structure s.  layers: the oracle's float32 [2][sum N][128]."""
    from oracle import oracle as orc
    _, layers = orc.egnn_embed(weights, pe, coords_list, return_layers=True)
    g_orc, p_orc = np.zeros(2), np.zeros(2)
    pos = 0
    for c, ref in zip(coords_list, refs):
        n = len(c)
        for layer in range(2):
            g, p = distances(layers[layer, pos:pos + n], ref[layer])
            g_orc[layer], p_orc[layer] = max(g_orc[layer], g), max(p_orc[layer], p)
        pos += n
    return g_orc, p_orc, layers
