"""The empty-ray skip (nerf_amd_ray_alive, include/nerf_amd.h) for the tests: the fp64 specification of the optical depth D of a proposal
histogram, of the alive flag and of the ordered compaction, in numpy.  Per ray, from the fp32 densities sigma_0 .. sigma_{C-1}, the fp32
ascending depths z_0 .. z_{C-1} and the direction d, everything in fp64:

    D     = |d| * sum_{s < C-1} max(sigma_s, 0) * (z_{s+1} - z_s)  +  max(sigma_{C-1}, 0) * 1e10        |d| = sqrt(dx^2 + dy^2 + dz^2)
    alive = !(D < D_min)

max keeps a NaN (the ray then stays alive); the closing delta is 1e10 and is not scaled by |d| (ProposalNetwork.get_weights).  The order of
the fp64 sum is not part of the definition: `undecidable` names the rays a different order may flip.  The keyword arguments of
`optical_depth`, `alive_flags` and `compact` plant the faults tests/test_skip_empty_host.py must see."""
import math

import numpy as np


def d_min_of_tau(tau: float) -> float:
    """the user-facing threshold: an opacity tau in (0, 1) -> D_min = -log1p(-tau), in double"""
    return -math.log1p(-float(tau))


def optical_depth(density, z, dirs, *, sum_dtype=np.float64, use_norm=True, closing="far", clamp=True):
    """density (N,C) fp32, z (N,C) fp32, dirs (N,3) fp32 -> D (N,) fp64.
    Faults: sum_dtype=np.float32 (an fp32 running sum); use_norm=False (the |d| factor dropped); closing="scaled" (the closing delta
    scaled by |d|) / "previous" (the previous interval taken as the closing delta); clamp=False (max(sigma, 0) dropped)."""
    sig = np.asarray(density, np.float32).astype(np.float64)
    zz = np.asarray(z, np.float32).astype(np.float64)
    d = np.asarray(dirs, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(sig < 0.0, 0.0, sig) if clamp else sig               # (a select, not np.maximum's NaN rules spelled out: NaN < 0 is False)
        terms = s[:, :-1] * (zz[:, 1:] - zz[:, :-1])
        if sum_dtype == np.float32:
            total = np.zeros(sig.shape[0], np.float32)
            for j in range(terms.shape[1]):
                total = (total + terms[:, j].astype(np.float32)).astype(np.float32)
            total = total.astype(np.float64)
        else:
            total = terms.sum(axis=1)
        nd = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if closing == "far":
            last = s[:, -1] * 1e10
        elif closing == "scaled":
            last = s[:, -1] * 1e10 * nd
        elif closing == "previous":
            last = s[:, -1] * (zz[:, -1] - zz[:, -2]) * nd
        else:
            raise ValueError(closing)
        return (nd if use_norm else 1.0) * total + last


def alive_flags(D, d_min, *, nan_alive=True):
    """!(D < D_min): a NaN stays alive.  Fault: nan_alive=False evaluates D >= D_min, which a NaN fails."""
    with np.errstate(invalid="ignore"):
        return ~(D < d_min) if nan_alive else (D >= d_min)


def compact(flags, *, ordered=True):
    """flags (N,) bool -> (row_of_ray (N,) int32: the rank among the alive rays or -1, ray_of_row (N',) int64 ascending, N').
    Fault: ordered=False hands out the rows in descending ray order (a valid permutation, as an atomic counter might produce)."""
    flags = np.asarray(flags, bool)
    ray_of_row = np.nonzero(flags)[0].astype(np.int64)
    if not ordered:
        ray_of_row = ray_of_row[::-1].copy()
    row_of_ray = np.full(flags.shape[0], -1, np.int32)
    row_of_ray[ray_of_row] = np.arange(ray_of_row.shape[0], dtype=np.int32)
    return row_of_ray, ray_of_row, int(ray_of_row.shape[0])


def spec(density, z, dirs, d_min):
    """-> dict(D, alive, row_of_ray, ray_of_row, n_alive)"""
    D = optical_depth(density, z, dirs)
    flags = alive_flags(D, d_min)
    row_of_ray, ray_of_row, n = compact(flags)
    return dict(D=D, alive=flags, row_of_ray=row_of_ray, ray_of_row=ray_of_row, n_alive=n)


def undecidable(D, d_min):
    """The rays whose flag the order of the fp64 summation may flip: |D - D_min| <= 1e-9 max(D, D_min).  (NaN and infinite D are decided.)"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(D) & np.isfinite(d_min) & (np.abs(D - d_min) <= 1e-9 * np.maximum(D, d_min))


# the device sweep's shapes (tests/test_gpu_skip_empty.py): one ray | a ragged wave-per-ray workgroup | one compaction wave | two tiles, the
# second ragged | four tiles; C: one interval | two | one chunk of 64 lanes | a second, one-element chunk | four chunks
GPU_N = (1, 63, 64, 257, 1000)
GPU_C = (2, 3, 64, 65, 256)


def make_inputs(N, C, seed, special=True):
    """density (N,C), z (N,C) ascending in (2, 6), dirs (N,3) of norms in about (0.3, 3): densities straddle 0; with `special`, rows (cyclic
    in the ray index) that are all negative, that have only the last density positive, that are large, and one all-NaN-free row with a single
    NaN; without, every row straddles 0."""
    rng = np.random.default_rng(1000 * seed + 17 * N + C)
    density = rng.normal(0.0, 1.0, (N, C)).astype(np.float32)
    z = np.sort(rng.uniform(2.0, 6.0, (N, C)).astype(np.float32), axis=1)
    dirs = (rng.normal(0.0, 1.0, (N, 3)) * rng.uniform(0.3, 3.0, (N, 1))).astype(np.float32)
    if special:
        for n in range(N):
            kind = n % 7
            if kind == 1:
                density[n] = -np.abs(density[n]) - 0.01
            elif kind == 3:
                density[n] = -np.abs(density[n]) - 0.01
                density[n, -1] = 1e-6
            elif kind == 5:
                density[n] *= 100.0
        density[N // 2, C // 2] = np.nan
    return density, z, dirs
