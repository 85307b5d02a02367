"""Restatement of the reference's mapping functions (slam/utils.py:25-38 depth_to_pcl with BackprojectDepth.forward of
layers.py:74-79 in front, :76-82 accumulate_pcl, :41-58 pcl_to_image), written from the rules in include/clslam_hip.h, in numpy.

``dtype=np.float64`` is the reference proper: the fp32 inputs are taken as exact and every operation after them runs in
float64.  ``dtype=np.float32`` is its twin: the arithmetic the reference does where its arrays are float32.  What both share are
the inputs as the kernel receives them (the distance threshold is a float32 number) and the PIXEL a point falls into, which the
rule fixes in float64 with individually rounded operations: zi = 1/z (1 for z = 0), u = (x zi) fx + cx, floor.

OpenCV is not installed where this project is developed, so the projection (cv2.projectPoints with zero rotation, translation
and distortion) is restated from OpenCV's source, not compared with cv2.
"""
import numpy as np

BAND = 2.0 ** -21           # relative distance below which an fp32 decision may differ from the float64 one


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def camera(H, W):
    """KITTI-like intrinsics: (K 3x3 float64, inv_K 4x4 float32)"""
    K = np.array([[0.58 * W, 0, 0.5 * W], [0, 0.96 * H, 0.5 * H], [0, 0, 1]], dtype=np.float64)
    inv = np.eye(4)
    inv[:3, :3] = np.linalg.inv(K)
    return K, inv.astype(np.float32)


def frame_pose(f):
    """world <- camera of frame f: 0.8 f m forward (z), 0.03 f rad of yaw (about y); float64"""
    a = 0.03 * f
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[2, 3] = 0.8 * f
    return T


def scene(H, W, frames, seed=0):
    """depth (F,1,H,W) = 3 + 57 r^2, image (F,3,H,W) uniform, inv_K (F,4,4) float32; K (3,3), poses (F,4,4) float64"""
    rng = np.random.default_rng(seed)
    depth = (3 + 57 * rng.random((frames, 1, H, W)) ** 2).astype(np.float32)
    image = rng.random((frames, 3, H, W)).astype(np.float32)
    K, inv = camera(H, W)
    return {'depth': depth, 'image': image, 'K': K, 'inv_K': np.repeat(inv[None], frames, 0),
            'poses': np.stack([frame_pose(f) for f in range(frames)])}


# ---- depth_to_pcl -------------------------------------------------------------------------------------------------------------
def backproject(depth, inv_K, image, dist_threshold=np.inf, dtype=np.float64):
    """one image: depth (H,W), inv_K (4,4), image (3,H,W) float32 -> {'all': (H W,6) rows of every pixel in pixel order, 'norm':
    (H W,) their distance, 'keep': (H W,) bool, 'points': the kept rows}, coordinates in `dtype`, colours float32 in 'colour'"""
    depth, inv_K, image = (np.asarray(a, dtype=np.float32) for a in (depth, inv_K, image))
    H, W = depth.shape
    ys, xs = np.divmod(np.arange(H * W), W)                                    # meshgrid(indexing='xy') flattened row-major
    pix = np.stack([xs, ys, np.ones(H * W)]).astype(dtype)
    cam = (depth.reshape(1, -1).astype(dtype) * (inv_K[:3, :3].astype(dtype) @ pix)).T
    norm = np.sqrt((cam * cam).sum(axis=1))
    thr = np.float32(dist_threshold)
    keep = np.ones(H * W, bool) if np.isinf(thr) else norm < dtype(thr)
    colour = image.reshape(3, -1).T
    return {'cam': cam, 'norm': norm, 'keep': keep, 'colour': colour, 'threshold': thr,
            'points': np.concatenate([cam[keep], colour[keep].astype(dtype)], axis=1)}


def threshold_band(norm64, thr):
    """the points whose float64 distance lies within BAND (relative) of the threshold"""
    if np.isinf(thr):
        return np.zeros(norm64.shape, bool)
    if thr == 0:
        return norm64 <= 0
    return np.abs(norm64 / np.float64(thr) - 1) <= BAND


# ---- accumulate_pcl -----------------------------------------------------------------------------------------------------------
def transform(points, offsets, poses, dtype=np.float64):
    """points (M,6) float32, offsets (F+1), poses (F,4,4) float64 -> ((M,3) coordinates in `dtype`, (M,3) the magnitude
    |R| |xyz| + |t| the rounding of the float64 evaluation scales with)"""
    points = np.asarray(points, dtype=np.float32)
    xyz = np.empty((points.shape[0], 3), dtype=dtype)
    mag = np.empty((points.shape[0], 3), dtype=np.float64)
    for f in range(len(offsets) - 1):
        a, b = int(offsets[f]), int(offsets[f + 1])
        T = np.asarray(poses[f], dtype=np.float64)
        p = points[a:b, :3]
        xyz[a:b] = p.astype(dtype) @ T[:3, :3].T.astype(dtype) + T[:3, 3].astype(dtype)
        mag[a:b] = np.abs(p.astype(np.float64)) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])
    return xyz, mag


def accumulate(pcl_list, pose_list, dtype=np.float64):
    out = []
    for pcl, T in zip(pcl_list, pose_list):
        xyz, _ = transform(pcl, [0, len(pcl)], [T], dtype)
        out.append(np.concatenate([xyz, np.asarray(pcl)[:, 3:].astype(dtype)], axis=1))
    return np.concatenate(out)


# ---- pcl_to_image -------------------------------------------------------------------------------------------------------------
def project(xyz, K, rows, cols, min_z=None):
    """xyz (M,3) float32 -> (M,) int64 pixel v * cols + u, -1 for the points that are skipped.  Always float64, every
    operation rounded on its own: this is the rule, not an approximation of it."""
    x, y, z = (np.asarray(xyz, dtype=np.float32)[:, i].astype(np.float64) for i in range(3))
    K = np.asarray(K, dtype=np.float64)
    with np.errstate(all='ignore'):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        zi = np.where(z != 0, 1.0 / np.where(z != 0, z, 1.0), 1.0)
        u = np.floor((x * zi) * K[0, 0] + K[0, 2])
        v = np.floor((y * zi) * K[1, 1] + K[1, 2])
        ok = finite & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
        if min_z is not None:
            ok &= z > min_z
        pix = np.where(ok, v * cols + u, -1)
    return np.where(ok, pix, -1).astype(np.int64)


def distance(xyz, dtype=np.float64):
    p = np.asarray(xyz, dtype=np.float32).astype(dtype)
    with np.errstate(all='ignore'):
        return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def zbuffer(points, K, image_shape, min_z=None, dtype=np.float64):
    """points (M,6) float32 -> dict of (rows,cols) planes: 'index' int64 (-1 empty) the closest point, the lowest index among
    equal distances; 'dist' its distance in `dtype` (+inf empty); 'image' (rows,cols,3) float32 its colour (0 empty); 'count'
    the candidates of the pixel; 'second' the distance of the runner-up (+inf: none).  'order' / 'start': the candidates of
    pixel p, closest first, are order[start[p]:start[p+1]].  Vectorised: lexsort on (pixel, distance, index)."""
    points = np.asarray(points, dtype=np.float32).reshape(-1, 6)
    rows, cols = int(image_shape[0]), int(image_shape[1])
    pix = project(points[:, :3], K, rows, cols, min_z)
    dist = distance(points[:, :3], dtype)
    cand = np.flatnonzero(pix >= 0)
    order = cand[np.lexsort((cand, dist[cand], pix[cand]))]
    count = np.bincount(pix[order], minlength=rows * cols)
    start = np.concatenate([[0], np.cumsum(count)])
    occupied = count > 0
    index = np.full(rows * cols, -1, dtype=np.int64)
    index[occupied] = order[start[:-1][occupied]]
    second = np.full(rows * cols, np.inf)
    two = count > 1
    second[two] = dist[order[start[:-1][two] + 1]]
    d = np.full(rows * cols, np.inf, dtype=dtype)
    d[occupied] = dist[index[occupied]]
    image = np.zeros((rows * cols, 3), dtype=np.float32)
    image[occupied] = points[index[occupied], 3:]
    return {'index': index.reshape(rows, cols), 'dist': d.reshape(rows, cols), 'image': image.reshape(rows, cols, 3),
            'count': count.reshape(rows, cols), 'second': second.reshape(rows, cols), 'order': order, 'start': start,
            'all_dist': dist, 'pix': pix}


def close_calls(z):
    """(rows,cols) bool: the pixels whose two closest candidates differ by less than BAND relative (float64 zbuffer)"""
    with np.errstate(all='ignore'):
        return (z['count'] > 1) & (z['second'] <= z['dist'].astype(np.float64) * (1 + BAND))


def in_band_candidates(z, p):
    """indices of the candidates of flat pixel p within BAND of the closest"""
    c = z['order'][z['start'][p]:z['start'][p + 1]]
    return c[z['all_dist'][c] <= z['all_dist'][c[0]] * (1 + BAND)]


def pcl_to_image_loop(pcl, camera_matrix, image_shape):
    """the reference's own shape of the computation: one Python iteration per point, a strict comparison against the running
    depth.  Slow; the check of the vectorised z-buffer and the 'per-point loop' row of tools/bench_map.py."""
    pcl = np.asarray(pcl, dtype=np.float32)
    pix = project(pcl[:, :3], camera_matrix, image_shape[0], image_shape[1])
    dist = distance(pcl[:, :3])
    image = np.zeros((image_shape[0] * image_shape[1], 3))
    depth = np.full(image_shape[0] * image_shape[1], np.inf)
    for i in range(pcl.shape[0]):
        p = pix[i]
        if p >= 0 and dist[i] < depth[p]:
            depth[p] = dist[i]
            image[p] = pcl[i, 3:]
    return image.reshape(image_shape[0], image_shape[1], 3)
