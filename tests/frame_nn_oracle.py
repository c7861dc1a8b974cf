"""numpy fp64 brute-force oracle of the frame neighbourhood searches (shine_mapping_amd.dataset.knn, statistical_outlier_mask,
estimate_normals; csrc/shine_frame_nn.hip): the full distance matrix, a stable argsort, open3d's definitions written out, and
numpy.linalg.eigh.  No scipy, no open3d.  tests/test_frame_nn.py checks the oracle itself on hand-built clouds."""
import numpy as np

SCENE_SEED = 20
SCENE_RADIUS, SCENE_MAX_NN, SCENE_K, SCENE_STD_RATIO = 0.2, 20, 25, 2.5  # the reference's defaults (utils/config.py)


def dist2_matrix(points):
    """[n,n] squared distances, (dx*dx + dy*dy) + dz*dz of the fp64 differences (each product and sum rounded once)"""
    p = np.asarray(points, dtype=np.float64)
    dx = p[:, None, 0] - p[None, :, 0]
    dy = p[:, None, 1] - p[None, :, 1]
    dz = p[:, None, 2] - p[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def sorted_neighbours(points):
    """(order int64 [n,n], d2 fp64 [n,n]): every row ascending by (squared distance, index) — the stable argsort's order"""
    d2 = dist2_matrix(points)
    order = np.argsort(d2, axis=1, kind="stable")
    return order, np.take_along_axis(d2, order, 1)


def knn(points, k, radius=None, sorted_=None):
    """-> (idx int32 [n,k] padded with -1, d2 [n,k] padded with +inf, count int32 [n]); the point itself is a neighbour"""
    order, d2 = sorted_ if sorted_ is not None else sorted_neighbours(points)
    n = order.shape[0]
    idx = np.full((n, k), -1, dtype=np.int32)
    out = np.full((n, k), np.inf)
    m = min(k, n)
    idx[:, :m], out[:, :m] = order[:, :m], d2[:, :m]
    if radius is not None:
        outside = ~(out <= float(radius) * float(radius))
        idx[outside], out[outside] = -1, np.inf
    return idx, out, (idx >= 0).sum(1).astype(np.int32)


def sor(points, nb_neighbors, std_ratio, sorted_=None):
    """open3d's remove_statistical_outlier: -> (keep bool [n], avg fp64 [n], threshold).  n == 1: std = 0."""
    _, d2, count = knn(points, nb_neighbors, None, sorted_)
    n = d2.shape[0]
    m = min(nb_neighbors, n)
    avg = np.sqrt(d2[:, :m]).sum(1) / m
    mean = avg.sum() / n
    std = np.sqrt(((avg - mean) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    threshold = mean + std_ratio * std
    return (avg > 0.0) & (avg < threshold), avg, float(threshold)


def normals(points, radius, max_nn, viewpoint=(0.0, 0.0, 0.0), sorted_=None):
    """open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) with every normal turned towards `viewpoint`:
    -> (normals fp64 [n,3], eigenvalues fp64 [n,3] ascending (NaN on fallback rows), count int32 [n], fallback bool [n]).
    Fallback (0, 0, 1) — before the flip — where count < 3 or the neighbours all coincide."""
    p = np.asarray(points, dtype=np.float64)
    idx, _, count = knn(p, max_nn, radius, sorted_)
    n = p.shape[0]
    out = np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))
    lam = np.full((n, 3), np.nan)
    fallback = np.ones(n, dtype=bool)
    for i in range(n):
        if count[i] < 3:
            continue
        q = p[idx[i, :count[i]]]
        c = q - q.mean(0)  # centred first: coordinates are tens of metres, neighbourhoods decimetres
        cov = c.T @ c
        if not np.trace(cov) > 0.0:
            continue
        w, v = np.linalg.eigh(cov)
        out[i] = v[:, 0] / np.linalg.norm(v[:, 0])
        lam[i] = w
        fallback[i] = False
    flip = (out * (np.asarray(viewpoint, dtype=np.float64) - p)).sum(1) < 0.0
    out[flip] = -out[flip]
    return out, lam, count, fallback


def relative_gap(lam):
    """(lambda1 - lambda0) / lambda2 per row: how well the smallest eigenvalue's direction is determined"""
    return (lam[:, 1] - lam[:, 0]) / lam[:, 2]


def scene(seed=SCENE_SEED):
    """The shared test cloud, [3945,3] fp64: three mutually orthogonal 4 m x 4 m faces (x = 0, y = 0, z = 0 of a corner) of 1300
    points each with 5 mm Gaussian noise off the face, shifted by (6, 5, -1.5) so that the sensor origin lies outside them; 40
    points uniform in +-20 m (the sparse outliers that force the unbounded search to widen); 5 exact duplicates of face points."""
    rng = np.random.default_rng(seed)
    faces = []
    for axis in range(3):
        f = rng.uniform(0.0, 4.0, (1300, 3))
        f[:, axis] = rng.normal(0.0, 0.005, 1300)
        faces.append(f)
    faces = np.concatenate(faces) + np.array([6.0, 5.0, -1.5])
    sparse = rng.uniform(-20.0, 20.0, (40, 3))
    dup = faces[rng.choice(len(faces), 5, replace=False)]
    return np.ascontiguousarray(np.concatenate([faces, sparse, dup]))


_SCENE = {}


def scene_results():
    """the scene and its oracle results, computed once per process and shared (treat as read-only)"""
    if not _SCENE:
        p = scene()
        s = sorted_neighbours(p)
        nrm, lam, count, fallback = normals(p, SCENE_RADIUS, SCENE_MAX_NN, sorted_=s)
        keep, avg, threshold = sor(p, SCENE_K, SCENE_STD_RATIO, sorted_=s)
        _SCENE.update(points=p, sorted=s, normals=nrm, lam=lam, count=count, fallback=fallback, keep=keep, avg=avg,
                      threshold=threshold)
    return _SCENE
