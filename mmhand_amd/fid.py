"""Frechet Inception Distance and Kernel Inception Distance of generated images against real ones, from the pooled [B,2048]
features of mmhand_amd.inception.InceptionV3 on the device.  The reference has neither metric; the definitions are those of
the two public implementations the published numbers come from:

* FID (pytorch-fid): mu = mean, sigma = np.cov(rowvar=False) of each set's features,
  |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr sqrt(S1 S2);
* KID (torch-fidelity): kernel k(x, y) = (x.y / d + 1)^3, the unbiased MMD^2 of random subsets of both sets, mean and standard
  deviation over the subsets.

The two reductions run on the device (csrc/fid.hip through ops.feature_moments and ops.poly_mmd_sums: fp64 MFMA, one fixed chain
per element, no atomics).  The trace of the matrix square root is taken once per evaluation on the host in float64
(frechet_distance) by a symmetric route: S1 = V diag(w) V^T, R = V sqrt(w+), M = R^T S2 R (symmetrised), tr sqrt(S1 S2) =
sum sqrt(lambda+(M)); in both decompositions eigenvalues below d 2^-52 lambda_max are set to zero first - under a square root
the rounding noise of a null space (fewer images than features) would otherwise enter at its square root's size.

Two departures from pytorch-fid, stated in DESIGN 4.5k: the resize to 299 is PIL's integer bilinear on bytes (the Inception
score's path; pytorch-fid interpolates floats), and tr sqrt comes from the symmetric route above instead of scipy's sqrtm.

No Inception weights ship with this repository: a figure means what its weight file (and variant) means."""
import warnings

import numpy as np
import torch

from . import ops
from .inception import SIZE, InceptionV3, PreprocessTables

KID_SUBSETS, KID_SUBSET_SIZE, KID_SEED = 100, 1000, 0


# ------------------------------------------------------------------------------------------------- host arithmetic
def _eigh_clipped(S):
    """eigenvalues (those below d 2^-52 lambda_max, negative ones included, set to zero) and eigenvectors of a symmetric matrix"""
    w, V = np.linalg.eigh(S)
    floor = S.shape[0] * 2.0 ** -52 * max(float(w[-1]), 0.0)
    return np.where(w < floor, 0.0, w), V


def frechet_distance(mu1, s1, mu2, s2):
    """-> {"fid", "mean_term", "trace_term", "tr_sqrt"}: fid = mean_term + trace_term, mean_term = |mu1 - mu2|^2,
    trace_term = tr(S1) + tr(S2) - 2 tr_sqrt, tr_sqrt = tr sqrt(S1 S2).  float64 on the host."""
    mu1, mu2 = np.asarray(mu1, dtype=np.float64).reshape(-1), np.asarray(mu2, dtype=np.float64).reshape(-1)
    s1, s2 = np.atleast_2d(np.asarray(s1, dtype=np.float64)), np.atleast_2d(np.asarray(s2, dtype=np.float64))
    d = mu1.shape[0]
    if mu2.shape != (d,) or s1.shape != (d, d) or s2.shape != (d, d):
        raise ValueError(f"frechet_distance: mu {mu1.shape} {mu2.shape}, sigma {s1.shape} {s2.shape}")
    w, V = _eigh_clipped((s1 + s1.T) * 0.5)
    R = V * np.sqrt(w)[None, :]
    M = R.T @ ((s2 + s2.T) * 0.5) @ R
    lam, _ = _eigh_clipped((M + M.T) * 0.5)
    tr_sqrt = float(np.sqrt(lam).sum())
    diff = mu1 - mu2
    mean_term = float(diff @ diff)
    trace_term = float(np.trace(s1)) + float(np.trace(s2)) - 2.0 * tr_sqrt
    return {"fid": mean_term + trace_term, "mean_term": mean_term, "trace_term": trace_term, "tr_sqrt": tr_sqrt}


def kid_from_sums(out, Ma, Mb):
    """out [S,3] of ops.poly_mmd_sums -> float64 [S]: the unbiased MMD^2 of every subset,
    sum_aa / (Ma (Ma - 1)) + sum_bb / (Mb (Mb - 1)) - 2 sum_ab / (Ma Mb)"""
    out = np.asarray(out, dtype=np.float64).reshape(-1, 3)
    if Ma < 2 or Mb < 2:
        raise ValueError(f"kid_from_sums: subsets of {Ma} and {Mb} rows: the unbiased estimate needs two of each")
    return out[:, 0] / (Ma * (Ma - 1.0)) + out[:, 1] / (Mb * (Mb - 1.0)) - 2.0 * out[:, 2] / (float(Ma) * Mb)


def draw_subsets(na, nb, subsets=KID_SUBSETS, subset_size=KID_SUBSET_SIZE, seed=KID_SEED):
    """-> (idxA int32 [S,M], idxB int32 [S,M]), M = min(subset_size, na, nb): per subset one draw without replacement from
    each set, A's before B's, from one np.random.RandomState(seed)"""
    if subsets < 1 or subset_size < 2:
        raise ValueError(f"draw_subsets: {subsets} subsets of {subset_size}")
    m = min(int(subset_size), int(na), int(nb))
    rng = np.random.RandomState(seed)
    ia, ib = np.empty((subsets, m), dtype=np.int32), np.empty((subsets, m), dtype=np.int32)
    for s in range(subsets):
        ia[s] = rng.choice(na, m, replace=False)
        ib[s] = rng.choice(nb, m, replace=False)
    return ia, ib


# ------------------------------------------------------------------------------------------------- statistics files
def save_stats(path, mu, sigma, n, variant, features=None):
    """an .npz with pytorch-fid's keys mu / sigma, plus n, variant and optionally the fp32 features (what KID needs)"""
    data = {"mu": np.asarray(mu, dtype=np.float64), "sigma": np.asarray(sigma, dtype=np.float64), "n": np.int64(n),
            "variant": np.str_(variant)}
    if features is not None:
        data["features"] = np.ascontiguousarray(features, dtype=np.float32)
    with open(path, "wb") as fh:        # np.savez on a name would append ".npz"
        np.savez(fh, **data)


def load_stats(path):
    """-> {"mu", "sigma", "n" (None in a file of pytorch-fid's), "variant" (None likewise), "features" (None if absent)}"""
    with np.load(path) as z:
        if "mu" not in z.files or "sigma" not in z.files:
            raise ValueError(f"{path}: no mu / sigma (keys {z.files})")
        mu, sigma = np.asarray(z["mu"], dtype=np.float64), np.asarray(z["sigma"], dtype=np.float64)
        if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
            raise ValueError(f"{path}: mu {mu.shape}, sigma {sigma.shape}")
        return {"mu": mu, "sigma": sigma, "n": int(z["n"]) if "n" in z.files else None,
                "variant": str(z["variant"]) if "variant" in z.files else None,
                "features": np.ascontiguousarray(z["features"], dtype=np.float32) if "features" in z.files else None}


# ------------------------------------------------------------------------------------------------- the scorer
class FidScorer:
    """feed_real() / feed_generated() enqueue preprocess -> InceptionV3.features and keep the fp32 [B,2048] rows on the device
    (8 KB an image); results() runs mmh_feature_moments on both sets, mmh_poly_mmd_sums on the subsets and on the full sets, and
    the host's frechet_distance.  set_real_stats() takes a statistics file's content in place of real images."""

    def __init__(self, net, variant="torchvision", device=None, size=SIZE, kid_subsets=KID_SUBSETS,
                 kid_subset_size=KID_SUBSET_SIZE, kid_seed=KID_SEED):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if not isinstance(net, InceptionV3):
            is_path = isinstance(net, (str, bytes)) or hasattr(net, "__fspath__")
            net = InceptionV3(self.device, variant=variant).load_state_dict(torch.load(net, map_location="cpu") if is_path else net)
        if net.variant != variant:
            raise ValueError(f"FidScorer: the network is the {net.variant!r} graph, asked for {variant!r}")
        draw_subsets(2, 2, kid_subsets, kid_subset_size, kid_seed)
        self.net, self.variant, self.size = net, variant, int(size)
        self.kid = (int(kid_subsets), int(kid_subset_size), int(kid_seed))
        self._tables, self._real, self._gen, self._stats = {}, [], [], None
        # for the caller's bookkeeping (evaluate): the network is an InceptionScorer's too / the real side is fed batch by batch
        self.shared, self.own_real = False, True

    def tables(self, H, W_):
        key = (int(H), int(W_))
        if key not in self._tables:
            self._tables[key] = PreprocessTables(H, W_, self.size, self.device, variant=self.variant)
        return self._tables[key]

    @torch.no_grad()
    def features(self, images, layout="nchw"):
        H, W_ = (images.shape[2], images.shape[3]) if layout == "nchw" else (images.shape[1], images.shape[2])
        return self.net.features(ops.inception_preprocess(images, layout, self.tables(H, W_)))

    def feed_real(self, images, layout="nchw"):
        self._real.append(self.features(images, layout))

    def feed_generated(self, images, layout="nchw", features=None):
        """features: the rows another consumer of the same forward already has (evaluate --inception --fid)"""
        self._gen.append(self.features(images, layout) if features is None else features)

    def set_real_stats(self, stats):
        """stats: load_stats()'s dict; its features, when present, serve KID"""
        if stats["variant"] is not None and stats["variant"] != self.variant:
            raise ValueError(f"FidScorer: statistics of the {stats['variant']!r} graph for a {self.variant!r} scorer")
        self._stats = stats
        if stats["features"] is not None:
            self._real = [torch.from_numpy(stats["features"]).to(self.device)]

    @staticmethod
    def _moments(X):
        mean, cov = ops.feature_moments(X)
        return mean.cpu().numpy(), cov.cpu().numpy()

    def _cat(self, parts, what):
        if not parts:
            return None
        X = torch.cat(parts).contiguous()
        if X.shape[0] < 2:
            raise ValueError(f"FidScorer: {X.shape[0]} {what} image(s): a covariance needs two")
        return X

    def results(self, stats_out=None):
        """{"FID", "KID_mean", "KID_std", "KID_full", "n_real", "n_generated", "fid_variant"} (+ "fid_terms": the parts of
        frechet_distance).  KID_* are None when the real side is a statistics file without features.  stats_out: a path for
        the real set's statistics (with features when they are at hand)."""
        G, R = self._cat(self._gen, "generated"), self._cat(self._real, "real")
        if G is None or (R is None and self._stats is None):
            raise ValueError("FidScorer: feed generated and real images (or set_real_stats) before results()")
        d = G.shape[1]
        mu_g, s_g = self._moments(G)
        if self._stats is None:
            mu_r, s_r = self._moments(R)
            n_real = int(R.shape[0])
        else:                               # a statistics file is the real side's mu and sigma; its features only serve KID
            mu_r, s_r, n_real = self._stats["mu"], self._stats["sigma"], self._stats["n"]
            if n_real is None and R is not None:
                n_real = int(R.shape[0])
        if mu_r.shape[0] != d:
            raise ValueError(f"FidScorer: real statistics of {mu_r.shape[0]} features, generated ones of {d}")
        if G.shape[0] < d or (n_real is not None and n_real < d):
            warnings.warn(f"FID from {G.shape[0]} generated and {n_real} real images of {d} features: fewer images than features - "
                          "the covariance is singular and FID is biased; KID is the figure to read", stacklevel=2)
        fd = frechet_distance(mu_g, s_g, mu_r, s_r)
        res = {"FID": fd["fid"], "KID_mean": None, "KID_std": None, "KID_full": None, "n_real": n_real,
               "n_generated": int(G.shape[0]), "fid_variant": self.variant, "fid_terms": fd}
        if R is not None:
            subsets, size, seed = self.kid
            ia, ib = draw_subsets(G.shape[0], R.shape[0], subsets, size, seed)
            kid = kid_from_sums(ops.poly_mmd_sums(G, R, ia, ib).cpu().numpy(), ia.shape[1], ib.shape[1])
            full = kid_from_sums(ops.poly_mmd_sums(G, R, np.arange(G.shape[0])[None], np.arange(R.shape[0])[None]).cpu().numpy(),
                                 G.shape[0], R.shape[0])
            res["KID_mean"], res["KID_std"], res["KID_full"] = float(np.mean(kid)), float(np.std(kid)), float(full[0])
        if stats_out:
            save_stats(stats_out, mu_r, s_r, n_real if n_real is not None else -1, self.variant,
                       None if R is None else R.cpu().numpy())
        return res
