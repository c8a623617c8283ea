"""The membrane fill of unet_watermark_amd.inpaint in numpy float32, operation by operation (include/uwm.h): pull,
push, `cycles` V-cycles of the multigrid on the hole, store.  It is the only thing the kernels are compared with, byte for byte.
Every array is float32 and every operation below is one rounded float32 operation; sums run in the stated order (neighbours: up,
left, right, down; children: (2Y, 2X), (2Y, 2X+1), (2Y+1, 2X), (2Y+1, 2X+1)), over the cells inside the level only, starting from
the first present."""
import numpy as np

F = np.float32
STATUS_FILLED, STATUS_NO_HOLE, STATUS_NO_KNOWN, STATUS_MISFIT = 0, 1, 2, 3


def num_levels(h, w):
    """L = ceil(log2(max(h, w))): level L is 1 x 1"""
    L = 0
    while (1 << L) < max(h, w):
        L += 1
    return L


def _ordered_sum(shape, terms):
    """terms: (destination slices, values) in order -> the sum over the present terms starting from the first present, their number"""
    s = np.zeros(shape, F)
    n = np.zeros(shape, np.int32)
    for dst, v in terms:
        started = n[dst] > 0
        s[dst] = np.where(started, s[dst] + v, v)
        n[dst] += 1
    return s, n


def neighbour_sum(u):
    a = slice(None)
    return _ordered_sum(u.shape, [((slice(1, None), a), u[:-1, :]), ((a, slice(1, None)), u[:, :-1]),
                                  ((a, slice(None, -1)), u[:, 1:]), ((slice(None, -1), a), u[1:, :])])


def children_sum(r, present):
    """r, present: level l -> per cell of level l + 1 the sum of r over the children that are in the level and `present`, in children
    order, and their number"""
    h, w = r.shape
    H, W = (h + 1) >> 1, (w + 1) >> 1
    s = np.zeros((H, W), F)
    n = np.zeros((H, W), np.int32)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        v, p = r[dy::2, dx::2], present[dy::2, dx::2]
        dst = (slice(0, v.shape[0]), slice(0, v.shape[1]))
        started = n[dst] > 0
        s[dst] = np.where(p, np.where(started, s[dst] + v, v), s[dst])
        n[dst] += p
    return s, n


def up(c, h, w):
    """the prolongation of the coarse plane c to h x w"""
    def axis(n, nc):
        y = np.arange(n)
        p = y >> 1
        q = np.clip(p + np.where(y & 1, 1, -1), 0, nc - 1)
        return p, q
    py, qy = axis(h, c.shape[0])
    px, qx = axis(w, c.shape[1])
    a, b = c[py][:, px], c[py][:, qx]
    d, e = c[qy][:, px], c[qy][:, qx]
    return ((F(9) * a + F(3) * b) + (F(3) * d + e)) * F(0.0625)


def sweep(u, b, unknown, parity):
    """one red-black sweep: the unknown cells with y + x even, then odd, each u = (b + S) / cnt"""
    for col in (0, 1):
        m = unknown & (parity == col)
        if m.any():
            s, n = neighbour_sum(u)
            u[m] = (b[m] + s[m]) / n[m].astype(F)


def residual(u, b, unknown):
    s, n = neighbour_sum(u)
    r = np.zeros(u.shape, F)
    r[unknown] = b[unknown] - (n[unknown].astype(F) * u[unknown] - s[unknown])
    return r


class Hierarchy:
    """what depends on the mask alone: the unknown sets H_l (= the non-valid cells of the pull), the parities"""

    def __init__(self, hole):
        h, w = hole.shape
        self.L = num_levels(h, w)
        self.H = [hole.astype(bool)]
        for _ in range(self.L):
            _, n = children_sum(np.zeros(self.H[-1].shape, F), ~self.H[-1])
            self.H.append(n == 0)
        self.parity = [np.add.outer(np.arange(m.shape[0]), np.arange(m.shape[1])) & 1 for m in self.H]
        self.levels_with_unknowns = int(sum(bool(m.any()) for m in self.H))


def pull_push(plane, hier):
    """plane: (h, w) float32, the bytes as floats -> u = g_0"""
    v = [plane.astype(F)]
    for l in range(hier.L):
        s, n = children_sum(v[-1], ~hier.H[l])
        with np.errstate(invalid="ignore", divide="ignore"):
            v.append(np.where(n > 0, s / n.astype(F), F(0)).astype(F))
    g = v[hier.L].copy()
    for l in range(hier.L - 1, -1, -1):
        g = np.where(hier.H[l], up(g, *v[l].shape), v[l]).astype(F)
        sweep(g, np.zeros(g.shape, F), hier.H[l], hier.parity[l])
    return g


def v_cycle(l, u, b, hier):
    Hl, par = hier.H[l], hier.parity[l]
    for _ in range(2):
        sweep(u, b, Hl, par)
    r = residual(u, b, Hl)
    if l < hier.L:
        b1, _ = children_sum(r, np.ones(r.shape, bool))
        b1[~hier.H[l + 1]] = 0
        e = np.zeros(b1.shape, F)
        v_cycle(l + 1, e, b1, hier)
        u[Hl] = u[Hl] + up(e, *u.shape)[Hl]
    for _ in range(2):
        sweep(u, b, Hl, par)


def solve_plane(plane, hier, cycles, trace=None):
    """one channel -> the float32 iterate after `cycles` V-cycles; trace: a list that receives a copy after the push and each cycle"""
    u = pull_push(plane, hier)
    if trace is not None:
        trace.append(u.copy())
    b = np.zeros(u.shape, F)
    for _ in range(cycles):
        v_cycle(0, u, b, hier)
        if trace is not None:
            trace.append(u.copy())
    return u


def inpaint_ref(image, mask, cycles):
    """image: uint8 (h, w, C) or (h, w); mask: (h, w), != 0 a hole pixel -> (the filled image, stats [hole pixels, status, levels that
    held unknowns, 0])"""
    image = np.asarray(image)
    mask = np.asarray(mask)
    assert image.dtype == np.uint8 and image.shape[:2] == mask.shape
    hole = mask != 0
    holes = int(hole.sum())
    if holes == 0:
        return image.copy(), [0, STATUS_NO_HOLE, 0, 0]
    if holes == hole.size:
        return image.copy(), [holes, STATUS_NO_KNOWN, 0, 0]
    hier = Hierarchy(hole)
    img3 = image.reshape(image.shape[0], image.shape[1], -1)
    out = img3.copy()
    for c in range(img3.shape[2]):
        u = solve_plane(img3[:, :, c].astype(F), hier, cycles)
        out[:, :, c][hole] = np.rint(np.minimum(np.maximum(u, F(0)), F(255)))[hole].astype(np.uint8)
    return out.reshape(image.shape), [holes, STATUS_FILLED, hier.levels_with_unknowns, 0]


def exact_membrane(plane, hole):
    """the level-0 linear system solved in float64: cnt u - S = 0 on the hole, u = the image elsewhere -> (h, w) float64"""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    h, w = hole.shape
    idx = -np.ones((h, w), np.int64)
    idx[hole] = np.arange(int(hole.sum()))
    ys, xs = np.nonzero(hole)
    rows, cols, vals = [], [], []
    rhs = np.zeros(len(ys))
    diag = np.zeros(len(ys))
    for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0)):
        y, x = ys + dy, xs + dx
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        diag += ok
        yy, xx, me = y[ok], x[ok], np.nonzero(ok)[0]
        unk = hole[yy, xx]
        rows.append(me[unk]); cols.append(idx[yy[unk], xx[unk]]); vals.append(-np.ones(int(unk.sum())))
        np.add.at(rhs, me[~unk], plane[yy[~unk], xx[~unk]].astype(np.float64))
    rows.append(np.arange(len(ys))); cols.append(np.arange(len(ys))); vals.append(diag)
    A = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(ys), len(ys)))
    out = plane.astype(np.float64).copy()
    out[hole] = spsolve(A.tocsc(), rhs)
    return out
