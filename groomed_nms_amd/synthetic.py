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


KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884],
                     [0.0, 0.0, 0.0, 1.0]])


def detection_heads(rng, B, A_grid=(32, 110, 36), n_objects=12, decomp_alpha=True, C=4, score_lo=0.0, score_hi=1.0, acceptance=True,
                    class_ties=True):
    """Network heads for the inference post-processing (detect.detections_from_heads) at the reference's configuration: A_grid = (H, W,
    anchors per cell) -> A = H * W * NA rois [A, 5] (x1 y1 x2 y2 tracker, stride 16), an anchor table [NA, 11], and per image head
    tensors whose DECODED boxes cluster KITTI-like: n_objects (<= 24) objects, one per cell of an 8 x 3 grid on the 1760 x 512 canvas
    and 12 m of depth apart, every anchor a proposal for one of them with a few per cent of jitter -- overlaps inside a cluster are
    high (2D IoU > 0.75), across clusters the 2D IoU is 0.  Scores are distinct by construction (a permutation of A levels between
    score_lo and score_hi); with class_ties about 1 % of the anchors repeat their best probability in a later class column, and the
    axis / head columns of some objects sit exactly on 0.5.  Head values are multiples of 2^-12.
    Returns dict(prob [B,A,C], bbox_2d [B,A,4], bbox_3d [B,A,10|7], acceptance [B,A,1] or None, rois, anchors, bbox_means [1,13],
    bbox_stds [1,13], p2 [4,4]), float32 heads."""
    H, W, NA = A_grid
    if not 1 <= n_objects <= 24:
        raise ValueError("n_objects must be in [1, 24]")
    wh = np.stack([rng.uniform(24, 200, NA), rng.uniform(24, 160, NA)], 1)
    a2 = np.concatenate([-wh / 2, wh / 2], 1)
    ys, xs = np.meshgrid(np.arange(H) * 16.0, np.arange(W) * 16.0, indexing="ij")
    sh = np.stack([xs.ravel(), ys.ravel(), xs.ravel(), ys.ravel()], 1)
    rois = np.concatenate([(sh[:, None] + a2[None]).reshape(-1, 4), np.tile(np.arange(NA), H * W)[:, None]], 1).astype(np.float32)
    A = rois.shape[0]
    anchors = np.zeros((NA, 11))
    anchors[:, :4] = a2
    anchors[:, 4] = rng.uniform(10, 40, NA)
    anchors[:, 5:8] = rng.uniform(1.0, 4.0, (NA, 3))
    anchors[:, 8:] = rng.uniform(-1, 1, (NA, 3))
    means = rng.normal(0, 0.1, (1, 13))
    stds = rng.uniform(0.2, 1.5, (1, 13))
    m32, s32 = means[0].astype(np.float32).astype(np.float64), stds[0].astype(np.float32).astype(np.float64)
    r64 = rois.astype(np.float64)
    widths = r64[:, 2] - r64[:, 0] + 1.0
    heights = r64[:, 3] - r64[:, 1] + 1.0
    ctr_x = r64[:, 0] + 0.5 * widths
    ctr_y = r64[:, 1] + 0.5 * heights
    src = anchors[rois[:, 4].astype(np.int64), 4:]

    def q(v):
        return (np.round(np.asarray(v) * 4096.0) / 4096.0).astype(np.float32)
    D3 = 10 if decomp_alpha else 7
    prob = np.zeros((B, A, C), np.float32)
    b2 = np.zeros((B, A, 4), np.float32)
    b3 = np.zeros((B, A, D3), np.float32)
    acc = np.zeros((B, A, 1), np.float32) if acceptance else None
    for b in range(B):
        cells = rng.permutation(24)[:n_objects]
        ocx = (cells % 8) * 220.0 + 110.0 + rng.uniform(-20, 20, n_objects)
        ocy = (cells // 8) * 170.0 + 85.0 + rng.uniform(-20, 20, n_objects)
        ow, oh = rng.uniform(40, 100, n_objects), rng.uniform(30, 80, n_objects)
        oz = 8.0 + 12.0 * rng.permutation(n_objects) + rng.uniform(0, 1, n_objects)
        odim = np.stack([rng.uniform(1.4, 2.0, n_objects), rng.uniform(1.3, 2.0, n_objects), rng.uniform(3, 5, n_objects)], 1)
        oal = rng.uniform(-2.5, 2.5, n_objects)
        oaxis = rng.choice([0.25, 0.5, 0.75], n_objects)                 # 0.5 itself: the reference's `>=`
        ohead = rng.choice([0.25, 0.5, 0.75], n_objects)
        ocls = rng.integers(1, C, n_objects)
        obj = rng.permutation(A) % n_objects
        cx = ocx[obj] + rng.uniform(-0.02, 0.02, A) * ow[obj]
        cy = ocy[obj] + rng.uniform(-0.02, 0.02, A) * oh[obj]
        pw = ow[obj] * np.exp(rng.uniform(-0.02, 0.02, A))
        ph = oh[obj] * np.exp(rng.uniform(-0.02, 0.02, A))
        d = np.stack([(cx - ctr_x) / widths, (cy - ctr_y) / heights, np.log(pw / widths), np.log(ph / heights)], 1)
        b2[b] = q((d - m32[:4]) / s32[:4])
        u = cx + rng.uniform(-1, 1, A)
        v = cy + rng.uniform(-1, 1, A)
        z = oz[obj] + rng.uniform(-0.03, 0.03, A)
        dim = odim[obj] * np.exp(rng.uniform(-0.01, 0.01, (A, 3)))
        al = oal[obj] + rng.uniform(-0.01, 0.01, A)
        t = np.zeros((A, D3))
        t[:, 0] = (u - ctr_x) / widths
        t[:, 1] = (v - ctr_y) / heights
        t[:, 2] = z - src[:, 0]
        t[:, 3:6] = np.log(dim / src[:, 1:4])
        t[:, :6] = (t[:, :6] - m32[4:10]) / s32[4:10]
        if decomp_alpha:
            ax, hd = oaxis[obj], ohead[obj]
            base = al - np.pi * (hd >= 0.5)
            sin_t = np.where(ax >= 0.5, base - src[:, 5], rng.uniform(-1, 1, A))
            cos_t = np.where(ax >= 0.5, rng.uniform(-1, 1, A), base - src[:, 6])
            t[:, 6] = (sin_t - m32[11]) / s32[11]
            t[:, 7] = (cos_t - m32[12]) / s32[12]
            t[:, 8] = ax
            t[:, 9] = hd
        else:
            t[:, 6] = ((al - src[:, 4]) - m32[10]) / s32[10]
        b3[b] = q(t)
        s = (score_lo + (score_hi - score_lo) * (rng.permutation(A) + 0.5) / A).astype(np.float32)
        p = (s[:, None] * (np.round(rng.uniform(0, 0.9, (A, C)) * 256.0) / 256.0)).astype(np.float32)
        p[np.arange(A), ocls[obj]] = s
        p[:, 0] = np.float32(1.0) - s
        if class_ties and C > 2:
            tie = np.flatnonzero((rng.random(A) < 0.01) & (ocls[obj] < C - 1))
            p[tie, ocls[obj][tie] + 1] = s[tie]
        prob[b] = p
        if acceptance:
            acc[b, :, 0] = np.round(rng.uniform(0.5, 1.0, A) * 65536.0) / 65536.0
    return dict(prob=prob, bbox_2d=b2, bbox_3d=b3, acceptance=acc, rois=rois, anchors=anchors, bbox_means=means, bbox_stds=stds, p2=KITTI_P2.copy())
