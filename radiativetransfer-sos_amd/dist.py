"""Multi-GPU sharding of the CKD-bin axis (one process per GPU, torch.distributed; backend "nccl" is RCCL
over xGMI on ROCm, "gloo" on CPU for tests).

The bin loop of SOS_PROC (src/SOS_PROC.F:3459-3594) is embarrassingly parallel: every rank solves a
contiguous slice of the bin list and forms its AIK-weighted partial sums locally; the only exchange is
ONE all-reduce(sum, fp64) per wavelength/band of the packed buffer
    [ (smax+1)*3*W Fourier records | 10 + N scalars (TDIFMUS, EMOINS, EPLUS, three transmissions, sum AIK,
      max / -min of the order counts, TDIFMUG(1..N)) ]
(~161 KB at N=41, 81 orders: latency-bound on xGMI), which replaces the serial file-based accumulation of
SOS_AGGREGATE (src/SOS_AGGREGATE.F:372-488).  The -ln of the three transmissions is applied after the
reduce (SOS_AGGREGATE.F:467-488).
"""
import numpy as np
import torch


def shard_range(nb, rank, world):
    """Contiguous slice [lo, hi) of nb bins for `rank` (sizes differ by at most one)."""
    base, rem = divmod(nb, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def bin_cost(tau_scat, tau_abs, fixed_levels=False):
    """Relative cost of one CKD bin on the solver, from what the host knows before any profile exists: the scattering optical
    depth of the wavelength (Rayleigh + aerosol) and the bin's total gas absorption optical depth.  Cost = levels x scattering
    steps: SOS_PROFILE lays a level every CTE_TCOUCHE = 0.005 of total optical depth between CTE_OS_NT_MIN = 100 and CTE_OS_NT
    = 600 levels, gas absorption counted up to CTE_THRESHOLD_TAUABS = 1.5 (SOS_PROFIL.F:349-361, 509-560; SOS.h:202-229,301);
    the number of scattering orders falls as absorption removes the multiply scattered light (fitted on the realistic mix:
    tests/test_dist_cpu.py checks the balance it gives against the true NT x orders of the oracle)."""
    ts = np.asarray(tau_scat, dtype=np.float64)
    tg = np.asarray(tau_abs, dtype=np.float64)
    # levels: 1.12 x (tau_scat + tau_gas) / 0.005 (the gas-aware placement adds ~12 % to the plain count), gas capped at 1.5
    # in a weak bin; a strong bin (tau_gas > 1.5) gets the levels of about one unit of gas; never below ~117
    nt = np.clip(1.12 * (ts + np.where(tg > 1.5, 1.0, tg)) / 0.005, 117.0, 600.0)
    steps = 1.0 / (1.0 + 0.12 * np.power(np.minimum(tg, 50.0), 0.7))
    if fixed_levels:                               # synthetic bands on one fixed level grid: only the scattering steps vary
        return steps + 0. * ts
    return nt * steps


def balanced_shards(costs, world):
    """Deal the items (CKD bins of a band, or wavelengths of a spectrum) to `world` ranks so that the summed cost per rank
    is even: longest-processing-time-first (items by decreasing cost, each to the least loaded rank; ties to the lower rank,
    so every rank computes the same partition).  Returns a list of `world` ascending index arrays -- within a rank the items
    keep their original order (the order SOS_PROC.F:3459-3466 enumerates the bins in), some may be empty.  The CKD bins of a
    band come strongest absorber first per gas, with NT 117...426 and 25...50 Fourier orders across a band: contiguous slices
    (shard_range) are off by 10-30 % there."""
    costs = np.asarray(costs, dtype=np.float64)
    load = np.zeros(world)
    owner = np.zeros(len(costs), dtype=np.int64)
    for i in np.argsort(-costs, kind="stable"):
        r = int(np.argmin(load))
        owner[i] = r
        load[r] += costs[i]
    return [np.nonzero(owner == r)[0] for r in range(world)]


def pack_partial(rec, scal):
    """rec [nseg][S][3][W], scal [nseg][10+N] -> one flat fp64 buffer per segment [nseg][S*3*W + 10 + N]."""
    nseg = rec.shape[0]
    return torch.cat([rec.reshape(nseg, -1), scal.reshape(nseg, -1)], dim=1).contiguous()


def unpack_partial(buf, rec_shape):
    nseg = buf.shape[0]
    n = int(np.prod(rec_shape[1:]))
    return buf[:, :n].reshape((nseg,) + tuple(rec_shape[1:])), buf[:, n:]


def all_reduce_partial(buf, n_scal, group=None):
    """Sum the packed partials over ranks (ONE fp64 all-reduce per band, SOS_AGGREGATE.F:372-459).  Elements 7 and 8 of
    the scalar block (max norders, -min norders) combine with MAX in a second, two-element collective.
    n_scal = width of the scalar block (10 + N)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return buf
    o = buf.shape[1] - n_scal
    mx = buf[:, o + 7:o + 9].clone()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    dist.all_reduce(mx, op=dist.ReduceOp.MAX, group=group)
    buf[:, o + 7:o + 9] = mx
    return buf


def finish_scalars(scal):
    """scal [nseg][10+N] (summed over all bins/ranks) -> dict of per-segment results as SOS_AGGREGATE leaves
    them: TDIFMUS, EMOINS, EPLUS, TTOT_TRONC, TTOT_VRAI, TAUOUT (-ln applied, SOS_AGGREGATE.F:467-488), sum(AIK),
    n_orders, min_orders (< 0: a bin failed, the reference's IER = -1), TDIFMUG[N]; tauvrai_out = -ln of element 9, the
    untruncated optical depth down to the slot's output altitude where sosgpu_level_transmission wrote it (inf where not)."""
    s = scal.detach().cpu().numpy() if isinstance(scal, torch.Tensor) else np.asarray(scal)
    return dict(tdifmus=s[:, 0], emoins=s[:, 1], eplus=s[:, 2], sum_aik=s[:, 6], n_orders=s[:, 7].astype(np.int32),
                tdifmug=s[:, 10:], **finish_depths(s[:, 3], s[:, 4], s[:, 5], s[:, 9], s[:, 8]))


def finish_depths(t_tronc, t_vrai, t_out, t_vrai_out, neg_min_orders):
    """The band values a scalar block holds as sums of transmissions, as SOS_AGGREGATE leaves them (-ln applied,
    SOS_AGGREGATE.F:467-488), and the failure flag: the one statement of these for finish_scalars (elements 3, 4, 5, 9 and 8
    of sosgpu_aggregate's block) and finish_irradiance (columns 6, 7, 8, 11 and 10 of sosgpu_level_irradiance's)."""
    with np.errstate(divide="ignore"):
        return dict(ttot_tronc=-np.log(t_tronc), ttot_vrai=-np.log(t_vrai), tauout=-np.log(t_out),
                    tauvrai_out=-np.log(t_vrai_out), min_orders=(-neg_min_orders).astype(np.int64))


def finish_irradiance(block):
    """block [nseg][capi.IRRADIANCE_COLS] of sosgpu_level_irradiance for one output slot -> the finish_scalars entries the
    flux rows read (ttot_tronc, ttot_vrai, tauout, tauvrai_out, min_orders, sum_aik), by finish_depths."""
    s = block.detach().cpu().numpy() if isinstance(block, torch.Tensor) else np.asarray(block)
    return dict(sum_aik=s[:, 9], **finish_depths(s[:, 6], s[:, 7], s[:, 8], s[:, 11], s[:, 10]))
