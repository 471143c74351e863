"""Data-adaptive knot initialisation on the device: the spherical Gaussian mixture behind `spatial_init_method: gmm`
(reference stnf/models/st_interp.py:187-266), fitted by stdadk_gmm_em_f64 -- one float64 EM iteration per call -- where
the host path calls sklearn.mixture.GaussianMixture(...).fit three times.

What stays on the host: the draw of the subsample (the same global-numpy-RNG call as the host path), the k-means++
seeding (sklearn's own public sklearn.cluster.kmeans_plusplus on one RandomState(42), three calls in sequence: exactly
what GaussianMixture(random_state=42, n_init=3, init_params='k-means++') does), the first M-step from the one-hot
responsibilities of the seeds (k rows), and the convergence test: one 8-byte read of the lower bound per iteration.

With seeding='device' the seeding moves too: the host draws only sklearn's random stream, which does not depend on the
data (kmeanspp_stream), and one stdadk_kmeanspp_f64 call per level runs the three restarts side by side
(kmeanspp_seeds_device).  The seeds are sklearn's in coordinates unless a pick is decided by the rounding of a sum -- a
threshold on a prefix-sum boundary, or two mutually nearest candidates whose potentials tie in exact arithmetic, which
becomes common only when k nears the number of distinct points (include/stdadk.h); seeding='host',
the default, stays bit for bit what it was.

`spatial_init_method: kmeans_balanced` (reference :345-431, which needs the k_means_constrained package) is fitted here
too, under the contract of include/stdadk.h: size-constrained k-means whose every assignment step is the exact optimum,
one stdadk_kmeans_balanced_iter_f64 call per iteration.  The knots are such a fit; they are NOT claimed to be the bits
that package would return.  On the host stay the subsample, the k-means++ seeds (the same three per level as above) and
the convergence test: one 16-byte read of {inertia, shift} and the 8-byte status per iteration; seeding='device' as above.
"""
import collections
import math

import numpy as np
import torch

from . import _native as N

EPS = float(np.finfo(np.float64).eps)
MAX_SAMPLES = 10000            # the reference's max_samples_for_gmm
N_INIT = 3
RANDOM_STATE = 42

GmmFit = collections.namedtuple("GmmFit", "weights means variances lower_bound n_iter best lower_bounds")
KMeansFit = collections.namedtuple("KMeansFit", "centers labels inertia n_iter best inertias")


def seed_parameters(points, idx, reg_covar):
    """The M-step from one-hot responsibilities on the seed rows, float64 numpy: nk = 1 + 10 eps, mu = x / nk,
    var = |x - mu|^2 / (d nk) + reg_covar, w = nk / n.  points (n, 2) float64, idx (k,) rows."""
    x = np.asarray(points, np.float64)[np.asarray(idx, np.int64)]
    nk = 1.0 + 10.0 * EPS
    mu = x / nk
    var = ((x - mu) ** 2).sum(axis=1) / (2.0 * nk) + reg_covar
    w = np.full(len(x), nk / len(points))
    return w, mu, var


def _check_points(who, points64, host_path):
    """`points64` is (n, 2) float64 on a HIP device, or `who` refuses it; `host_path` says where the host path is."""
    if points64.dtype != torch.float64 or points64.dim() != 2 or points64.shape[1] != 2:
        raise RuntimeError(f"{who}: points must be (n, 2) float64, got {points64.dtype} {tuple(points64.shape)}")
    if not points64.is_cuda:
        raise RuntimeError(f"{who}: points must live on a HIP device (cuda:N), got {points64.device}; {host_path}")


def _seed_rows(who, r, idx, k, unit):
    """The k seed rows of restart r as an int64 array."""
    idx = np.asarray(idx, np.int64)
    if idx.shape != (k,):
        raise ValueError(f"{who}: restart {r} has {idx.shape} seeds, {k} {unit} expected")
    return idx


def fit_spherical_gmm(points64, n_components, seed_indices, max_iter=100, tol=1e-3, reg_covar=1e-6):
    """EM for a spherical mixture of `n_components` Gaussians on points64 ((n, 2) float64 on a HIP device), one restart
    per index array of `seed_indices` (the k rows whose one-hot responsibilities start it), as GaussianMixture.fit
    with warm_start=False: from lb = -inf, each iteration is one stdadk_gmm_em_f64 call (E on the current parameters,
    then M) and stops when |lb - prev| < tol; the restart with the largest lower bound is kept, the first on a tie.
    Returns GmmFit(weights (k,), means (k, 2), variances (k,) float64 device tensors, lower_bound, per-restart n_iter,
    the chosen restart, per-restart lower bounds)."""
    _check_points("fit_spherical_gmm", points64, "the host path is sklearn's (init_device=None)")
    if len(seed_indices) == 0:
        raise ValueError("fit_spherical_gmm: no restart given")
    points64 = points64.contiguous()
    dev, n, k = points64.device, points64.shape[0], int(n_components)
    host = points64.cpu().numpy()
    ws = torch.empty(N.gmm_workspace_bytes(n, k) // 8, device=dev, dtype=torch.float64)
    lb_dev = torch.empty(1, device=dev, dtype=torch.float64)
    new = lambda: (torch.empty(k, device=dev, dtype=torch.float64), torch.empty(k, 2, device=dev, dtype=torch.float64),
                   torch.empty(k, device=dev, dtype=torch.float64))                        # noqa: E731
    best, best_lb, best_params, n_iters, lbs = -1, -math.inf, None, [], []
    with torch.cuda.device(dev):
        for r, idx in enumerate(seed_indices):
            idx = _seed_rows("fit_spherical_gmm", r, idx, k, "components")
            cur = tuple(torch.from_numpy(a).to(dev) for a in seed_parameters(host, idx, reg_covar))
            nxt = new()
            lb, it = -math.inf, 0
            for it in range(1, max_iter + 1):
                prev = lb
                N.gmm_em(points64, cur[0], cur[1], cur[2], reg_covar, nxt[0], nxt[1], nxt[2], lb_dev, ws)
                cur, nxt = nxt, cur
                lb = float(lb_dev.item())
                if abs(lb - prev) < tol:
                    break
            n_iters.append(it)
            lbs.append(lb)
            if lb > best_lb or best < 0:
                best, best_lb, best_params = r, lb, cur
    return GmmFit(best_params[0], best_params[1], best_params[2], best_lb, n_iters, best, lbs)


def grid_bandwidth(k):
    """Bandwidth of the uniform grid with k knots: 2.5 x spacing (the reference's clipping yardstick)."""
    side = int(math.sqrt(k))
    return 2.5 * (1.0 / (side - 1) if side > 1 else 1.0)


def knots_from_fit(means64, variances64, k):
    """(centres (k, 2), bandwidths (k,)) float32 from a level's float64 fit: bandwidth = 4.23 * 2.5 * sigma, floored at a
    quarter of the same-size grid's bandwidth (numpy, as the host path)."""
    bw = np.clip(4.23 * 2.5 * np.sqrt(np.asarray(variances64, np.float64)), 0.25 * grid_bandwidth(k), float('inf'))
    return torch.from_numpy(np.asarray(means64, np.float64)).float(), torch.from_numpy(bw).float()


def subsample(train_coords):
    """At most MAX_SAMPLES rows, drawn with the global numpy RNG exactly as the host path draws them, as float64."""
    pts = np.asarray(train_coords)
    if len(pts) > MAX_SAMPLES:
        pts = pts[np.random.choice(len(pts), MAX_SAMPLES, replace=False)]
    return pts.astype(np.float64)


def kmeanspp_seeds(points, n_centers):
    """Per level the N_INIT k-means++ index arrays of GaussianMixture(random_state=42, n_init=3,
    init_params='k-means++'): every level starts a fresh RandomState(42), its restarts draw from it in sequence."""
    from sklearn.cluster import kmeans_plusplus
    out = []
    for k in n_centers:
        rs = np.random.RandomState(RANDOM_STATE)
        out.append([kmeans_plusplus(points, k, random_state=rs)[1] for _ in range(N_INIT)])
    return out


def kmeanspp_trials(k):
    """Candidates per further centre: sklearn's n_local_trials = 2 + floor(ln k)."""
    return 2 + int(np.log(k))


def kmeanspp_stream(n, n_centers):
    """The random numbers behind kmeanspp_seeds, which do not depend on the points: per level (first (N_INIT,) int32,
    u (N_INIT, k - 1, L) float64) with L = kmeanspp_trials(k).  Every level opens a fresh RandomState(42); per restart,
    in sequence, the first row is drawn as sklearn's _kmeans_plusplus draws it for unit weights, then L uniforms for each
    of the k - 1 further centres."""
    out = []
    p = np.ones(n, dtype=np.float64) / float(n)
    for k in n_centers:
        rs = np.random.RandomState(RANDOM_STATE)
        L = kmeanspp_trials(k)
        first, u = np.empty(N_INIT, np.int32), np.empty((N_INIT, k - 1, L), np.float64)
        for r in range(N_INIT):
            first[r] = rs.choice(n, p=p)
            u[r] = rs.uniform(size=(k - 1, L))         # the same numbers as k - 1 draws of L, in one call
        out.append((first, u))
    return out


def kmeanspp_seeds_device(points64, n_centers):
    """kmeanspp_seeds with the data-dependent part on the device: points64 (n, 2) float64 on a HIP device; per level one
    stdadk_kmeanspp_f64 call with runs = N_INIT on the stream of kmeanspp_stream and one read of the N_INIT x k rows."""
    _check_points("kmeanspp_seeds_device", points64, "kmeanspp_seeds is the host path")
    points64 = points64.contiguous()
    dev, n = points64.device, points64.shape[0]
    for k in n_centers:
        if not 1 <= k <= min(n, N.KMEANSPP_MAX_K):
            raise ValueError(f"kmeanspp_seeds_device: {k} seeds on {n} points (1 <= k <= min(n, {N.KMEANSPP_MAX_K}))")
    out = []
    with torch.cuda.device(dev):
        for k, (first, u) in zip(n_centers, kmeanspp_stream(n, n_centers)):
            idx = torch.empty(N_INIT, k, device=dev, dtype=torch.int32)
            pot = torch.empty(N_INIT, device=dev, dtype=torch.float64)
            ws = torch.empty(N.kmeanspp_workspace_bytes(n, k, N_INIT) // 8, device=dev, dtype=torch.float64)
            N.kmeanspp(points64, torch.from_numpy(first).to(dev), torch.from_numpy(u).to(dev), idx, pot, ws)
            out.append(list(idx.cpu().numpy().astype(np.int64)))
    return out


SEEDINGS = ('host', 'device')


def seeds_by_level(pts, pts_dev, n_centers, seeding):
    """The N_INIT seed index arrays of every level, by sklearn on the host or by the kernel on the points' device."""
    return kmeanspp_seeds(pts, n_centers) if seeding == 'host' else kmeanspp_seeds_device(pts_dev, n_centers)


def _knots_on_device(who, host_path, train_coords, n_centers, device, seeding, level_knots, admit=lambda n, k: None):
    """What gmm_knots and balanced_kmeans_knots share.  The subsample is drawn first, then the seeds (both may draw from
    the global numpy RNG); admit(n, k) may refuse a level before anything reaches the device; level_knots(points on the
    device, k, the level's seeds) -> (centres (k, 2), bandwidths (k,)) float32 host tensors, concatenated in list order."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"{who}: a HIP device (cuda:N) is required, got {device}; {host_path}")
    if seeding not in SEEDINGS:
        raise ValueError(f"{who}: seeding must be one of {SEEDINGS}, got {seeding!r}")
    pts = subsample(train_coords)
    for k in n_centers:
        admit(len(pts), k)
    pts_dev = torch.from_numpy(pts).to(device)
    seeds = seeds_by_level(pts, pts_dev, n_centers, seeding)
    cs, bs = zip(*[level_knots(pts_dev, k, level_seeds) for k, level_seeds in zip(n_centers, seeds)])
    return torch.cat(cs, dim=0), torch.cat(bs, dim=0)


def gmm_knots(train_coords, n_centers, device, seeding='host'):
    """The reference's _init_gmm with the mixture fitted on `device`: (centres (sum k, 2), bandwidths (sum k,)) float32
    host tensors, levels concatenated in list order.  seeding: 'host' = sklearn's kmeans_plusplus, 'device' = the same
    random stream through stdadk_kmeanspp_f64."""
    def level(pts_dev, k, level_seeds):
        fit = fit_spherical_gmm(pts_dev, k, level_seeds, max_iter=100, tol=1e-3, reg_covar=1e-6)
        return knots_from_fit(fit.means.cpu().numpy(), fit.variances.cpu().numpy(), k)
    return _knots_on_device("gmm_knots", "init_device=None is the host path", train_coords, n_centers, device, seeding, level)


def balanced_bounds(n, k):
    """(lo, hi) cluster sizes of a level of k knots on n points (reference :379-385)."""
    if k > n:
        raise ValueError(f"kmeans_balanced: {k} knots need at least {k} points, got {n}")
    return max(1, n // k - 1), n // k + n % k


def fit_balanced_kmeans(points64, k, seed_indices, max_iter=100, tol_factor=1e-4, history=None):
    """Size-constrained k-means with `k` clusters on points64 ((n, 2) float64 on a HIP device), one restart per index
    array of `seed_indices` (the k rows the centres start at).  Each iteration is one stdadk_kmeans_balanced_iter_f64
    call (the exact assignment under lo <= |cluster| <= hi, then the means) and stops when the centres' squared shift is
    at most tol_factor x mean(var(points, axis 0)); the restart with the lowest inertia is kept, the first on a tie.
    Returns KMeansFit(centers (k, 2) float64 and labels (n,) int32 device tensors, inertia, per-restart n_iter, the
    chosen restart, per-restart inertias).  `history`, a list, receives per restart the list of (inertia, shift,
    augmentations) of every iteration."""
    _check_points("fit_balanced_kmeans", points64, "there is no host path (it needs the k_means_constrained package)")
    if len(seed_indices) == 0:
        raise ValueError("fit_balanced_kmeans: no restart given")
    points64 = points64.contiguous()
    dev, n, k = points64.device, points64.shape[0], int(k)
    lo, hi = balanced_bounds(n, k)
    host = points64.cpu().numpy()
    tol = tol_factor * float(np.mean(np.var(host, axis=0)))
    ws = torch.empty(N.kmeans_workspace_bytes(n, k) // 8, device=dev, dtype=torch.float64)
    stats = torch.empty(2, device=dev, dtype=torch.float64)
    status = torch.empty(2, device=dev, dtype=torch.int32)
    best, best_inertia, best_out, n_iters, inertias = -1, math.inf, None, [], []
    with torch.cuda.device(dev):
        for r, idx in enumerate(seed_indices):
            idx = _seed_rows("fit_balanced_kmeans", r, idx, k, "clusters")
            cur = torch.from_numpy(host[idx]).to(dev)
            nxt = torch.empty_like(cur)
            labels = torch.empty(n, device=dev, dtype=torch.int32)
            trace, it, inertia = [], 0, math.inf
            for it in range(1, max_iter + 1):
                N.kmeans_balanced_iter(points64, cur, lo, hi, nxt, labels, stats, status, ws)
                cur, nxt = nxt, cur
                inertia, shift = stats.tolist()
                code, n_aug = status.tolist()
                if code != 0:
                    raise RuntimeError(f"fit_balanced_kmeans: the assignment of restart {r}, iteration {it} stopped on a "
                                       f"bound (status {code}: {N.KMEANS_STATUS.get(code, '?')}) after {n_aug} augmentations")
                trace.append((inertia, shift, n_aug))
                if shift <= tol:
                    break
            n_iters.append(it)
            inertias.append(inertia)
            if history is not None:
                history.append(trace)
            if best < 0 or inertia < best_inertia:
                best, best_inertia, best_out = r, inertia, (cur, labels)
    return KMeansFit(best_out[0], best_out[1], best_inertia, n_iters, best, inertias)


def neighbour_bandwidths(centers, k, k0):
    """Bandwidths (k,) of scattered knots, numpy: 2.5 x the mean distance to the min(4, k - 1) nearest other centres of
    the level; the grid bandwidth of k0 (= n_centers[0]) knots for k == 1 (reference :320-341 and :400-422, the same
    arithmetic behind random_site and kmeans_balanced)."""
    from scipy.spatial.distance import cdist
    dist = cdist(centers, centers)
    np.fill_diagonal(dist, np.inf)
    nn = min(4, k - 1) if k > 1 else 1
    bw = 2.5 * np.sort(dist, axis=1)[:, :nn].mean(axis=1)
    if k == 1:
        bw = np.array([grid_bandwidth(k0)])
    return bw


def balanced_kmeans_knots(train_coords, n_centers, device, seeding='host'):
    """The reference's _init_kmeans_balanced with the fit of fit_balanced_kmeans on `device`: (centres (sum k, 2),
    bandwidths (sum k,)) float32 host tensors, levels concatenated in list order.  seeding as in gmm_knots."""
    def level(pts_dev, k, level_seeds):
        c = fit_balanced_kmeans(pts_dev, k, level_seeds).centers.cpu().numpy()
        return torch.from_numpy(c).float(), torch.from_numpy(neighbour_bandwidths(c, k, n_centers[0])).float()
    return _knots_on_device("balanced_kmeans_knots", "without init_device the initialiser needs the k_means_constrained "
                            "package", train_coords, n_centers, device, seeding, level, admit=balanced_bounds)
