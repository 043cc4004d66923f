"""Plain per-pixel loops for the topology-aware centreline loss `cldice` (the rule of include/eosvos.h at EOSVOS_LOSS_CLDICE),
and the inputs its tests share.  The loops follow the rule pixel by pixel: the selections with their tie rules, the skeleton
product, the gathers of the backward pass in their order.  The reductions over an image (four sums) are numpy's sum over the
valid pixels in row-major order, the same call the vectorised twin makes: a sum's order is no part of the rule.  Imported as a
plain module by tests/test_cldice_host.py and tests/test_gpu_cldice.py."""
import numpy as np

# (images, H, W, depth): tile seams of 32 x 8 and 64 x 16 with remainders both ways, the largest depth, one row, two columns
CASES = [(2, 19, 37, 3), (1, 33, 70, 5), (1, 40, 45, 16), (1, 1, 9, 2), (1, 5, 2, 2), (1, 7, 7, 1)]
IGN = 255.0


def lattice(images, H, W, seed):
    """Logits: a random permutation of n equally spaced values over [-4, 4].  Neighbours are 8 / n apart, so p orders alike
    in float32 and float64 and only exact ties occur."""
    n = images * H * W
    rng = np.random.default_rng(seed)
    return np.linspace(-4.0, 4.0, n)[rng.permutation(n)].reshape(images, H, W).astype(np.float32)


def target(images, H, W):
    """A thin cross and a small block per image, float32 in {0, 1}."""
    y = np.zeros((images, H, W), dtype=np.float32)
    for b in range(images):
        y[b, H // 2, W // 6:W - W // 6] = 1
        y[b, :, (W // 3 + b) % W] = 1
        y[b, H // 5:H // 5 + max(1, H // 4), (2 * W) // 3:(2 * W) // 3 + max(1, W // 5)] = 1
    return y


def case(images, H, W, seed=0):
    return lattice(images, H, W, seed), target(images, H, W)


def void_ring(z, y, rows=2, cols=3, seed=1):
    """The frame padded by a ring of void pixels with arbitrary logits: (z, y, the boolean map of the inner frame)."""
    B, H, W = z.shape
    rng = np.random.default_rng(seed)
    zz = rng.uniform(-30, 30, (B, H + 2 * rows, W + 2 * cols)).astype(np.float32)
    yy = np.full(zz.shape, IGN, dtype=np.float32)
    inner = np.zeros(zz.shape, dtype=bool)
    inner[:, rows:rows + H, cols:cols + W] = True
    zz[inner] = z.reshape(-1)
    yy[inner] = y.reshape(-1)
    return zz, yy, inner


def speckle(y, seed=2, share=0.1):
    """The targets with a random tenth of the pixels void; the middle one where the draw left none (the smallest frames)."""
    rng = np.random.default_rng(seed)
    out = y.copy()
    out[rng.random(y.shape) < share] = IGN
    if not (out == IGN).any():
        out.reshape(-1)[out.size // 2] = IGN
    return out


def bar_and_blob():
    """A 24 x 40 target with a 2-pixel bar and a 6 x 8 blob, and two predictions four pixels short of it: the bar cut through,
    the blob's edge shaved.  Returns (y, cut, shave) as float32 maps in {0, 1}."""
    y = np.zeros((24, 40), dtype=np.float32)
    y[4:6, 3:37] = 1
    y[12:18, 14:22] = 1
    cut, shave = y.copy(), y.copy()
    cut[4:6, 19:21] = 0
    shave[12, 16:20] = 0
    return y, cut, shave


# ---- the loops -----------------------------------------------------------------------------------------------------------------
VERTICAL = ((-1, 0), (0, 0), (1, 0))
HORIZONTAL = ((0, -1), (0, 0), (0, 1))
SQUARE = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
CROSS = ((-1, 0), (0, -1), (0, 0), (0, 1), (1, 0))


def first(x, valid, r, c, offsets, fill, less):
    """(the first extremum over the valid pixels of the window, its index in `offsets`; the centre's without any)."""
    H, W = x.shape
    m, arg = fill, offsets.index((0, 0))
    for n, (dy, dx) in enumerate(offsets):
        rr, cc = r + dy, c + dx
        if 0 <= rr < H and 0 <= cc < W and valid[rr, cc]:
            v = x[rr, cc]
            if (v < m) if less else (v > m):
                m, arg = v, n
    return m, arg


def chain_loops(x, valid, depth):
    """One (H, W) map: (S, [d_j], [(av, ah, which, ad)_j]) in the dtype of x."""
    dt = x.dtype.type
    H, W = x.shape
    u = np.ones((H, W), dtype=x.dtype)
    ds, routes = [], []
    for _ in range(depth + 1):
        nxt = np.zeros((H, W), dtype=x.dtype)
        av, ah, wh, ad = (np.zeros((H, W), dtype=np.int8) for _ in range(4))
        for r in range(H):
            for c in range(W):
                if valid[r, c]:
                    v, av[r, c] = first(x, valid, r, c, VERTICAL, dt(np.inf), True)
                    h, ah[r, c] = first(x, valid, r, c, HORIZONTAL, dt(np.inf), True)
                    wh[r, c] = 0 if v < h else 1 if h < v else 2
                    nxt[r, c] = h if h < v else v
        d = np.zeros((H, W), dtype=x.dtype)
        for r in range(H):
            for c in range(W):
                if valid[r, c]:
                    o, ad[r, c] = first(nxt, valid, r, c, SQUARE, dt(-np.inf), False)
                    t = dt(x[r, c] - o)
                    d[r, c] = t if t > 0 else dt(0)
                    u[r, c] = dt(u[r, c] * dt(dt(1) - d[r, c]))
        ds.append(d)
        routes.append((av, ah, wh, ad))
        x = nxt
    return np.where(valid, dt(1) - u, dt(0)).astype(x.dtype), ds, routes


def backward_loops(gs, ds, routes, valid):
    """T_0 of one (H, W) map from g_S by the gathers of the rule."""
    dt = gs.dtype.type
    H, W = gs.shape
    k1 = len(ds)
    gd = []
    for j in range(k1):
        g = np.zeros((H, W), dtype=gs.dtype)
        for r in range(H):
            for c in range(W):
                if valid[r, c] and ds[j][r, c] > 0:
                    e = dt(1)
                    for m in range(k1):
                        if m != j:
                            e = dt(e * dt(dt(1) - ds[m][r, c]))
                    g[r, c] = dt(gs[r, c] * e)
        gd.append(g)

    def gather3(t, j, r, c):
        for n, (dy, dx) in enumerate(SQUARE):
            rr, cc = r + dy, c + dx
            hit = 0 <= rr < H and 0 <= cc < W and valid[rr, cc] and routes[j][3][rr, cc] == 8 - n
            t = dt(t - (gd[j][rr, cc] if hit else dt(0)))
        return t

    t = np.zeros((H, W), dtype=gs.dtype)
    for r in range(H):
        for c in range(W):
            if valid[r, c]:
                t[r, c] = gather3(dt(0), k1 - 1, r, c)
    for j in range(k1 - 1, -1, -1):
        av, ah, wh, _ = routes[j]
        nt = np.zeros((H, W), dtype=gs.dtype)
        for r in range(H):
            for c in range(W):
                if not valid[r, c]:
                    continue
                a = gd[j][r, c]
                for dy, dx in CROSS:
                    rr, cc = r + dy, c + dx
                    w = dt(0)
                    if 0 <= rr < H and 0 <= cc < W and valid[rr, cc]:
                        if dx == 0 and av[rr, cc] == 1 - dy:
                            w = dt(w + (dt(1) if wh[rr, cc] == 0 else dt(0.5) if wh[rr, cc] == 2 else dt(0)))
                        if dy == 0 and ah[rr, cc] == 1 - dx:
                            w = dt(w + (dt(1) if wh[rr, cc] == 1 else dt(0.5) if wh[rr, cc] == 2 else dt(0)))
                        a = dt(a + dt(w * t[rr, cc]))
                    else:
                        a = dt(a + dt(0))
                if j >= 1:
                    a = gather3(a, j - 1, r, c)
                nt[r, c] = a
        t = nt
    return t


def skeleton_loops(x, depth, valid=None, dtype=np.float32):
    """S of (images, H, W) maps by the loops."""
    x = np.asarray(x)
    valid = np.ones(x.shape, dtype=bool) if valid is None else valid
    x = np.where(valid, x, 0).astype(dtype)
    return np.stack([chain_loops(x[b], valid[b], depth)[0] for b in range(x.shape[0])])


def loss_loops(z, y, depth, ignore=None, dtype=np.float64):
    """(loss, gradient) of (images, H, W) logits and targets by the loops, every intermediate in `dtype`."""
    from eosvos_amd import cldice
    dt = np.dtype(dtype).type
    valid = np.ones(y.shape, dtype=bool) if ignore is None else y != np.float32(ignore)
    B = z.shape[0]
    with np.errstate(invalid='ignore'):
        z = np.where(valid, z, 0).astype(dt)
        y = np.where(valid, y, 0).astype(dt)
        p, pq = cldice.sigmoid_host(z, dt)
        loss, grad = dt(0), np.zeros(z.shape, dtype=dt)
        for b in range(B):
            m = valid[b]
            if not m.any():
                continue
            sp, ds, routes = chain_loops(p[b], m, depth)
            sy = chain_loops(y[b], m, depth)[0]
            sums = [a[m].sum(dtype=dt) for a in (sp * y[b], sp, sy * p[b], sy)]
            li, tp, c1, c2 = cldice.coefficients(sums, dt)
            loss = loss + li
            gs = np.where(m, c1 * (y[b] - tp), dt(0)).astype(dt)
            t0 = backward_loops(gs, ds, routes, m)
            grad[b] = np.where(m, (t0 + np.where(m, c2 * sy, dt(0))) * pq[b] / dt(B), dt(0))
    return dt(loss / dt(B)), grad


# ---- the published implementation (Shit et al. 2021) on torch's CPU ops, for the fp64 check ------------------------------------
def published(z, y, depth):
    """(loss, gradient) by torch autograd in float64, the mean over the images of the per-image loss; no void label."""
    import torch
    import torch.nn.functional as F

    def erode(img):
        return torch.min(-F.max_pool2d(-img, (3, 1), (1, 1), (1, 0)), -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1)))

    def dilate(img):
        return F.max_pool2d(img, (3, 3), (1, 1), (1, 1))

    def skel(img):
        s = F.relu(img - dilate(erode(img)))
        for _ in range(depth):
            img = erode(img)
            delta = F.relu(img - dilate(erode(img)))
            s = s + F.relu(delta - s * delta)
        return s

    zt = torch.tensor(np.asarray(z, dtype=np.float64), requires_grad=True)
    yt = torch.tensor(np.asarray(y, dtype=np.float64))
    total = 0
    for b in range(zt.shape[0]):
        p, t = torch.sigmoid(zt[b])[None, None], yt[b][None, None]
        sp, st = skel(p), skel(t)
        tp = ((sp * t).sum() + 1) / (sp.sum() + 1)
        ts = ((st * p).sum() + 1) / (st.sum() + 1)
        total = total + 1 - 2 * tp * ts / (tp + ts)
    total = total / zt.shape[0]
    total.backward()
    return float(total.detach()), zt.grad.numpy()
