"""Seeded synthetic inputs for the parity tests and bench.py (SURVEY.md 8-d generators).

uniform-2D:   centres U([0,1760]x[0,512]), w,h ~ U(16,136)   (canvas = crop_size, scripts/config/groumd_nms.py:91)
clustered-2D: K = N/per objects, each replicated `per` times with centre jitter N(0, 0.1*size) and
              log-size jitter N(0, 0.1) -- KITTI-like: many proposals per object, groups near the cap
3D:           x~U(-30,30), y~U(0.5,2.5), z~U(5,60), l~U(3,5), w~U(1.4,2), h~U(1.3,2), ry~U(-pi,pi)
scores:       U(0,1) fp32, distinct by construction (the reference's order among ties is unspecified)
"""
import numpy as np


def uniform_boxes_2d(rng, n):
    c = np.stack([rng.uniform(0, 1760, n), rng.uniform(0, 512, n)], 1)
    wh = rng.uniform(16, 136, size=(n, 2))
    return np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)


def clustered_boxes_2d(rng, n, per=64):
    k = max(1, n // per)
    base = uniform_boxes_2d(rng, k).astype(np.float64)
    bc = (base[:, :2] + base[:, 2:]) / 2
    bs = base[:, 2:] - base[:, :2]
    which = np.arange(n) % k
    c = bc[which] + rng.normal(0, 0.1, size=(n, 2)) * bs[which]
    s = bs[which] * np.exp(rng.normal(0, 0.1, size=(n, 2)))
    out = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)
    return out[rng.permutation(n)]


def boxes_3d(rng, n, clustered=False, per=64):
    def draw(m):
        return np.stack([rng.uniform(-30, 30, m), rng.uniform(0.5, 2.5, m), rng.uniform(5, 60, m),
                         rng.uniform(1.4, 2.0, m), rng.uniform(1.3, 2.0, m), rng.uniform(3, 5, m),
                         rng.uniform(-np.pi, np.pi, m)], 1)   # x y z w h l ry
    if not clustered:
        return draw(n).astype(np.float32)
    k = max(1, n // per)
    base = draw(k)
    which = np.arange(n) % k
    p = base[which].copy()
    p[:, :3] += rng.normal(0, 0.15, size=(n, 3))
    p[:, 3:6] *= np.exp(rng.normal(0, 0.05, size=(n, 3)))
    p[:, 6] += rng.normal(0, 0.05, size=n)
    return p[rng.permutation(n)].astype(np.float32)


def tie_free_scores(rng, n, lo=0.0, hi=1.0):
    s = rng.uniform(lo, hi, size=n).astype(np.float32)
    # argsort-rank perturbation: nudge duplicates apart by ulps until all distinct
    for _ in range(64):
        u, idx, cnt = np.unique(s, return_index=True, return_counts=True)
        if len(u) == n:
            return s
        dup = np.ones(n, bool)
        dup[idx] = False
        s[dup] = np.nextafter(s[dup], np.float32(hi), dtype=np.float32)
    raise RuntimeError("could not make scores distinct")


def batch_2d(seed, B, N, kind="uniform", per=64):
    """(boxes [B,N,4], scores [B,N]) fp32."""
    rng = np.random.default_rng(seed)
    gen = uniform_boxes_2d if kind == "uniform" else (lambda r, n: clustered_boxes_2d(r, n, per))
    boxes = np.stack([gen(rng, N) for _ in range(B)])
    scores = np.stack([tie_free_scores(rng, N) for _ in range(B)])
    return boxes, scores


def batch_3d(seed, B, N, clustered=True, per=64):
    rng = np.random.default_rng(seed)
    params = np.stack([boxes_3d(rng, N, clustered, per) for _ in range(B)])
    scores = np.stack([tie_free_scores(rng, N) for _ in range(B)])
    return params, scores


def anchor_scene(rng, B, Mmax=256, Kmax=8, dtype=np.float32, D3=16, acols=11, garbage=True):
    """Anchor target assignment at the reference's configuration (crop 512 x 1760, stride 16, 36 anchors): B images of
    R = 32 * 110 * 36 = 126 720 rois [B, R, 5] (x1 y1 x2 y2 tracker) with ragged ground truths padded to Mmax / Kmax rows.  Padding
    rows hold NaN (labels -7) when garbage.  Returns dict(rois, gv [B, Mmax, 4], gi [B, Kmax, 4], g3 [B, Mmax, D3], lb [B, Mmax], Mc,
    Kc, anchors [36, acols], r3 [B, R, acols] (rois_3d), cen [B, R, 2])."""
    H, W, A = 32, 110, 36
    wh = np.stack([rng.uniform(12, 300, A), rng.uniform(12, 200, A)], 1)
    a2 = np.concatenate([-wh / 2, wh / 2], 1)
    ys, xs = np.meshgrid(np.arange(H) * 16.0, np.arange(W) * 16.0, indexing="ij")
    sh = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], 1)
    rois = np.concatenate([(sh[:, None] + a2[None]).reshape(-1, 4), np.tile(np.arange(A), H * W)[:, None]], 1)
    R = rois.shape[0]
    anchors = np.zeros((A, acols))
    anchors[:, :4] = a2
    anchors[:, 4] = rng.uniform(5, 40, A)
    anchors[:, 5:8] = rng.uniform(0.5, 4, (A, 3))
    anchors[:, 8:] = rng.uniform(-2, 2, (A, acols - 8))
    rb = np.repeat(rois[None], B, 0) + np.concatenate([rng.normal(0, 2, (B, R, 4)), np.zeros((B, R, 1))], 2)
    rb = rb.astype(dtype)
    Mc = rng.integers(0, Mmax + 1, B)
    Mc[0] = Mmax
    Kc = rng.integers(0, Kmax + 1, B)
    fill = np.nan if garbage else 0.0
    gv = np.full((B, Mmax, 4), fill)
    gi = np.full((B, Kmax, 4), fill)
    g3 = np.full((B, Mmax, D3), fill)
    lb = np.full((B, Mmax), -7 if garbage else 1, np.int32)
    for b in range(B):
        m = Mc[b]
        pick = rng.choice(R, m, replace=False)
        g = rb[b, pick, :4].astype(np.float64) + rng.normal(0, 8, (m, 4))
        g[:, 2:] = np.maximum(g[:, 2:], g[:, :2] + 4)
        gv[b, :m] = g
        lb[b, :m] = rng.integers(1, 4, m)
        g3[b, :m] = np.concatenate([rng.uniform(0, 1760, (m, 2)), rng.uniform(5, 50, (m, 1)), rng.uniform(0.5, 4, (m, 3)),
                                    rng.uniform(-3, 3, (m, D3 - 6))], 1)
        k = Kc[b]
        gi[b, :k] = rb[b, rng.choice(R, k), :4].astype(np.float64) + rng.normal(0, 20, (k, 4))
    r3 = np.concatenate([rb[..., :4], anchors[rois[:, 4].astype(np.int64), 4:][None].repeat(B, 0) + rng.normal(0, 0.05, (B, R, acols - 4))],
                        2).astype(dtype)
    cen = ((rb[..., :2] + rb[..., 2:4]) / 2).astype(dtype)
    return dict(rois=rb, gv=gv, gi=gi, g3=g3, lb=lb, Mc=Mc, Kc=Kc, anchors=anchors, r3=r3, cen=cen)
