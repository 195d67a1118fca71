"""Host-side mirror of the slice of Molly.jl's API that fronts the nonbonded hot path.

Julia is not available in this image, so this module stands where `MollyHIPExt.jl` stands in
a Julia session: same names, argument meaning and error behaviour as the reference, calling the same C ABI.
Indices are 0-based here (Python), 1-based in Julia.

Reference interfaces mirrored (Molly.jl v0.23.3):
  System                      src/types.jl:795-979
  Atom                        src/types.jl:466-475
  CubicBoundary               src/spatial.jl:40
  NoCutoff … PolynomialCutoff src/cutoffs.jl:53-253
  LennardJones                src/interactions/lennard_jones.jl:25-47
  Coulomb / CoulombReactionField / CoulombEwald   src/interactions/coulomb.jl:32, 698, 1320
  DistanceNeighborFinder / GPUNeighborFinder      src/neighbors.jl:104-115, 376-388
  NeighborList                src/types.jl:611-654
  forces / potential_energy / kinetic_energy / temperature   src/force.jl:670-720, src/energy.jl:86-248
  find_neighbors              src/neighbors.jl:390-423
  VelocityVerlet, simulate!   src/simulators.jl:287-300, 547-668
  remove_CM_motion!           src/spatial.jl:901-929
"""
import ctypes as C
import math
import warnings
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import MollyHipError

COULOMB_CONST = 138.93545764   # coulomb.jl:16, kJ mol^-1 nm e^-2
BOLTZMANN = 8.314462618e-3     # kJ mol^-1 K^-1 (setup.jl:2007)


# ---- cutoffs (cutoffs.jl) ---------------------------------------------------------------------------
@dataclass(frozen=True)
class NoCutoff:
    kind = _lib.CUTOFF_NONE
    dist_cutoff: float = 0.0
    dist_activation: float = 0.0


@dataclass(frozen=True)
class DistanceCutoff:
    dist_cutoff: float
    kind = _lib.CUTOFF_DISTANCE
    dist_activation: float = 0.0


@dataclass(frozen=True)
class ShiftedPotentialCutoff:
    dist_cutoff: float
    kind = _lib.CUTOFF_SHIFTED_POTENTIAL
    dist_activation: float = 0.0


@dataclass(frozen=True)
class ShiftedForceCutoff:
    dist_cutoff: float
    kind = _lib.CUTOFF_SHIFTED_FORCE
    dist_activation: float = 0.0


class _TwoRadiusCutoff:
    def __init__(self, dist_activation, dist_cutoff):
        if dist_cutoff <= dist_activation:   # cutoffs.jl:180-183, 234-237
            raise ValueError(f"the cutoff radius {dist_cutoff} must be larger than the activation radius {dist_activation}")
        self.dist_activation, self.dist_cutoff = float(dist_activation), float(dist_cutoff)


class CubicSplineCutoff(_TwoRadiusCutoff):
    kind = _lib.CUTOFF_CUBIC_SPLINE


class PolynomialCutoff(_TwoRadiusCutoff):
    kind = _lib.CUTOFF_POLYNOMIAL


# ---- pairwise interactions ----------------------------------------------------------------------------
@dataclass
class LennardJones:
    """LennardJones(; cutoff, use_neighbors, weight_special) with Lorentz σ / geometric ϵ mixing and the
    LJZeroShortcut (the defaults, lennard_jones.jl:29-34)."""
    cutoff: object = field(default_factory=NoCutoff)
    use_neighbors: bool = False
    weight_special: float = 1.0


@dataclass
class Coulomb:
    cutoff: object = field(default_factory=NoCutoff)
    use_neighbors: bool = False
    weight_special: float = 1.0
    coulomb_const: float = COULOMB_CONST


@dataclass
class CoulombReactionField:
    dist_cutoff: float
    solvent_dielectric: float = 78.3   # coulomb.jl:705 crf_solvent_dielectric
    use_neighbors: bool = False
    weight_special: float = 1.0
    coulomb_const: float = COULOMB_CONST


class CoulombEwald:
    def __init__(self, dist_cutoff, error_tol=0.0005, use_neighbors=False, weight_special=1.0,
                 coulomb_const=COULOMB_CONST, approximate_erfc=True, dtype=np.float64):
        self.dist_cutoff, self.error_tol = float(dist_cutoff), float(error_tol)
        self.use_neighbors, self.weight_special, self.coulomb_const = use_neighbors, float(weight_special), float(coulomb_const)
        self.approximate_erfc = bool(approximate_erfc)
        T = np.dtype(dtype).type
        # α = inv(dist_cutoff) * sqrt(-log(2 * error_tol)) evaluated in T (coulomb.jl:1332)
        self.α = float((T(1) / T(dist_cutoff)) * np.sqrt(-np.log(T(2) * T(error_tol))))


def use_neighbors(inter):
    return inter.use_neighbors


class PME:
    """PME(dist_cutoff, atoms, boundary; error_tol=0.0005, order=5, ϵr=1.0): reciprocal-space part of the particle-mesh Ewald
    sum, a general interaction (ewald.jl:361-421).  α and the mesh are derived as the reference does (:368-369, :479-482)."""

    def __init__(self, dist_cutoff, atoms=None, boundary=None, error_tol=0.0005, order=5, ϵr=1.0, dtype=np.float64):
        if boundary is None:
            raise ValueError("PME needs the boundary")
        T = np.dtype(dtype).type
        self.dist_cutoff, self.error_tol, self.order, self.ϵr = float(dist_cutoff), float(error_tol), int(order), float(ϵr)
        self.α = float((T(1) / T(dist_cutoff)) * np.sqrt(-np.log(T(2) * T(error_tol))))
        sides = boundary.side_lengths if isinstance(boundary, (CubicBoundary, TriclinicBoundary)) else tuple(boundary)      # box_sides(boundary), spatial.jl:357-360
        tol = T(error_tol)
        self.mesh_dims = tuple(max(int(np.ceil(T(2) * T(self.α) * T(L) / (T(3) * tol ** T(0.2)))), 6) for L in sides)   # pme_params


# ---- specific interaction lists (SoA form of InteractionList{2,3,4}Atoms, types.jl:236-420) ---------
@dataclass
class HarmonicBonds:
    i: np.ndarray; j: np.ndarray; k: np.ndarray; r0: np.ndarray


@dataclass
class HarmonicAngles:
    i: np.ndarray; j: np.ndarray; k: np.ndarray; kθ: np.ndarray; θ0: np.ndarray


@dataclass
class PeriodicTorsions:
    """One entry per (torsion, Fourier term); proper and improper torsions may share one list."""
    i: np.ndarray; j: np.ndarray; k: np.ndarray; l: np.ndarray
    periodicity: np.ndarray; phase: np.ndarray; k0: np.ndarray


@dataclass
class EwaldExclusions:
    i: np.ndarray; j: np.ndarray


# ---- boundary / atoms / neighbour finder ------------------------------------------------------------
class CubicBoundary:
    def __init__(self, x, y=None, z=None):
        if y is None:
            sl = np.broadcast_to(np.asarray(x, dtype=np.float64), (3,)).copy()
        else:
            sl = np.array([x, y, z], dtype=np.float64)
        if np.any(sl <= 0):   # spatial.jl:46-48
            raise ValueError("CubicBoundary side lengths must be positive")
        self.side_lengths = sl


class TriclinicBoundary:
    """TriclinicBoundary(v1, v2, v3; approx_images=true) (spatial.jl:131-220): v1 along x, v2 in the xy plane, v3.z > 0.  The engine
    supports it on a single GPU, PME included (include/mollyhip.h, mhip_set_triclinic)."""

    def __init__(self, v1, v2, v3, approx_images=True):
        bv = np.array([v1, v2, v3], dtype=np.float64).reshape(3, 3)
        if not (bv[0, 0] > 0) or bv[0, 1] != 0 or bv[0, 2] != 0:   # spatial.jl:173-177
            raise ValueError(f"first basis vector must be along the x-axis (no y or z component) and have a positive x component, got {bv[0]}")
        if not (bv[1, 1] > 0) or bv[1, 2] != 0:                     # :178-182
            raise ValueError(f"second basis vector must be in the xy plane (no z component) and have a positive y component, got {bv[1]}")
        if not (bv[2, 2] > 0):                                      # :183-186
            raise ValueError(f"third basis vector must have a positive z component, got {bv[2]}")
        self.basis_vectors = bv
        self.approx_images = bool(approx_images)
        self.side_lengths = np.array([bv[0, 0], bv[1, 1], bv[2, 2]])     # box_volume = v1.x · v2.y · v3.z; the engine's config box
        self.reciprocal_size = 1.0 / self.side_lengths


@dataclass
class Atom:
    index: int = 0
    atom_type: int = 0
    mass: float = 1.0
    charge: float = 0.0
    σ: float = 0.0
    ϵ: float = 0.0
    λ: float = 1.0


class NeighborList:
    """n entries (i, j, special), i < j, 0-based."""
    def __init__(self, i, j, special):
        self.i, self.j, self.special = i, j, special
        self.n = len(i)

    @property
    def list(self):
        return list(zip(self.i.tolist(), self.j.tolist(), self.special.astype(bool).tolist()))


def _pairs_from(arg, name):
    """Accepts a dense boolean matrix (as Molly's eligible/special) or an (m,2) array of pairs."""
    if arg is None:
        return np.zeros((0, 2), np.int32)
    a = np.asarray(arg)
    if a.dtype == bool and a.ndim == 2 and a.shape[0] == a.shape[1]:
        ii, jj = np.nonzero(np.triu(a, 1) | np.triu(a.T, 1))
        return np.stack([ii, jj], 1).astype(np.int32)
    a = a.reshape(-1, 2).astype(np.int64)
    if len(a) and (a.min() < 0):
        raise ValueError(f"{name}: negative atom index")
    lo, hi = np.minimum(a[:, 0], a[:, 1]), np.maximum(a[:, 0], a[:, 1])
    keep = lo != hi
    # normalize_pairs: i<j, sorted, unique (neighbors.jl:171-195)
    u = np.unique(np.stack([lo[keep], hi[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    return u.astype(np.int32)


class GPUNeighborFinder:
    """GPUNeighborFinder(; eligible, dist_cutoff, special, n_steps_reorder) — neighbors.jl:104-115, 320-361.
    `eligible`/`special` may be dense Bool matrices or sparse pair arrays (`excluded_pairs`, `special_pairs`)."""
    def __init__(self, dist_cutoff, eligible=None, special=None, excluded_pairs=None, special_pairs=None, n_steps=10):
        self.dist_cutoff = float(dist_cutoff)
        self.n_steps = int(n_steps)
        if eligible is not None:
            el = np.asarray(eligible, dtype=bool)
            excluded_pairs = np.argwhere(np.triu(~el | ~el.T, 1))
        self.excluded = _pairs_from(excluded_pairs, "excluded_pairs")
        self.special = _pairs_from(special if special is not None else special_pairs, "special_pairs")


DistanceNeighborFinder = GPUNeighborFinder       # same contract for this engine (neighbors.jl:376-388)
CellListMapNeighborFinder = GPUNeighborFinder    # neighbors.jl:543-590


class NoNeighborFinder:
    dist_cutoff = math.inf
    n_steps = 10
    excluded = np.zeros((0, 2), np.int32)
    special = np.zeros((0, 2), np.int32)


@dataclass
class VelocityVerlet:
    dt: float
    coupling: object = None
    remove_CM_motion: int = 1    # simulators.jl:293


@dataclass
class SteepestDescentMinimizer:
    """SteepestDescentMinimizer(; step_size=0.01 nm, max_steps=1000, tol=1000 kJ mol⁻¹ nm⁻¹) (simulators.jl:112-135): x += hn · F / max|F|, the step taken when
    the potential energy falls (hn · 6/5) and taken back otherwise (hn / 5), until max|F| < tol.
    engine_loop=True runs the loop in the engine (mhip_minimize), which also takes constrained Systems — every constrained pair a harmonic bond of
    constraint_bond_constant [kJ mol⁻¹ nm⁻²] for the duration, None: the constraints ignored (constraints_to_bonds, constraints.jl:619-636) — and virtual sites"""
    step_size: float = 0.01
    max_steps: int = 1000
    tol: float = 1000.0
    log_stream: object = None
    constraint_bond_constant: object = 500_000.0
    engine_loop: bool = False


@dataclass
class AndersenThermostat:
    """AndersenThermostat(temperature, coupling_const) (coupling.jl:188-211): every step each atom's velocity is re-drawn from the
    Maxwell-Boltzmann distribution with probability dt / coupling_const."""
    temperature: float
    coupling_const: float


@dataclass
class ImmediateThermostat:
    """ImmediateThermostat(temperature) (coupling.jl:68-91): every step the velocities are scaled by λ = sqrt(T₀ / T)."""
    temperature: float


@dataclass
class BerendsenThermostat:
    """BerendsenThermostat(temperature, coupling_const) (coupling.jl:214-238): λ² = 1 + (dt / coupling_const)·(T₀ / T − 1) every step."""
    temperature: float
    coupling_const: float


@dataclass
class VelocityRescaleThermostat:
    """VelocityRescaleThermostat(temperature, coupling_const; n_steps=1) (coupling.jl:93-168): Bussi's stochastic velocity rescaling, applied every
    n_steps steps with the time step dt·n_steps."""
    temperature: float
    coupling_const: float
    n_steps: int = 1


_RESCALE_KIND = {ImmediateThermostat: 1, BerendsenThermostat: 2, VelocityRescaleThermostat: 3}      # mhip_set_thermostat


class Langevin:
    """Langevin(; dt, temperature, friction, coupling=nothing, remove_CM_motion=1) — the Langevin middle integrator
    (simulators.jl:1065-1097): vel_scale = exp(−dt·friction), noise_scale = sqrt(1 − vel_scale²)."""

    def __init__(self, dt, temperature, friction, coupling=None, remove_CM_motion=1):
        self.dt, self.temperature, self.friction = float(dt), float(temperature), float(friction)
        self.coupling, self.remove_CM_motion = coupling, int(remove_CM_motion)
        self.vel_scale = float(np.exp(-self.dt * self.friction))
        self.noise_scale = float(np.sqrt(1.0 - self.vel_scale ** 2))


class LangevinSplitting:
    """LangevinSplitting(; dt, temperature, friction, splitting, remove_CM_motion=1) (simulators.jl:1212-1253): a sequence of A (drift), B (kick) and O
    (friction + noise) sub-steps, e.g. "BAOAB".  friction is a mass per time, as in the reference.  coupling: nothing or AndersenThermostat (this package's addition)."""

    def __init__(self, dt, temperature, friction, splitting, remove_CM_motion=1, coupling=None):
        self.dt, self.temperature, self.friction = float(dt), float(temperature), float(friction)
        self.splitting, self.remove_CM_motion, self.coupling = str(splitting), int(remove_CM_motion), coupling


class OverdampedLangevin:
    """OverdampedLangevin(; dt, temperature, friction, remove_CM_motion=1) (simulators.jl:1400-1424): Euler–Maruyama; friction is an inverse time."""

    def __init__(self, dt, temperature, friction, remove_CM_motion=1):
        self.dt, self.temperature, self.friction = float(dt), float(temperature), float(friction)
        self.remove_CM_motion, self.coupling = int(remove_CM_motion), None


@dataclass
class DistanceConstraint:
    """DistanceConstraint(i, j, dist) (constraints.jl:7-18): atoms i and j (0-based) held at distance dist (nm)"""
    i: int
    j: int
    dist: float


class AngleConstraint:
    """AngleConstraint(i, j, k, angle_ijk, dist_ij, dist_jk) (constraints.jl:38-53): a rigid triangle around the central atom j, held as its three
    distances; dist_ik follows from the law of cosines.  A linear angle cannot be constrained."""

    def __init__(self, i, j, k, angle_ijk, dist_ij, dist_jk):
        c = math.cos(angle_ijk)
        if c == -1:
            raise ValueError(f"disallowed linear angle constraint found between atoms {i}/{j}/{k}")
        self.i, self.j, self.k = int(i), int(j), int(k)
        self.dist_ij, self.dist_jk = float(dist_ij), float(dist_jk)
        self.dist_ik = math.sqrt(dist_ij ** 2 + dist_jk ** 2 - 2 * dist_ij * dist_jk * c)


class SHAKE_RATTLE:
    """SHAKE_RATTLE(; n_atoms, dist_tolerance=1e-8 nm, vel_tolerance=1e-8 nm² ps⁻¹, dist_constraints, angle_constraints, max_iters=25) (shake.jl:6-96).
    The clusters are built, checked and run by the engine (mhip_set_constraints): RATTLE after every kick, SHAKE after every drift."""

    def __init__(self, n_atoms, dist_tolerance=1e-8, vel_tolerance=1e-8, dist_constraints=None, angle_constraints=None, max_iters=25):
        if not dist_tolerance > 0:
            raise ValueError("dist_tolerance must be greater than zero")
        if not vel_tolerance > 0:
            raise ValueError("vel_tolerance must be greater than zero")
        self.n_atoms = int(n_atoms)
        self.dist_tolerance, self.vel_tolerance, self.max_iters = float(dist_tolerance), float(vel_tolerance), int(max_iters)
        self.dist_constraints = list(dist_constraints or ())
        self.angle_constraints = list(angle_constraints or ())

    @property
    def n_constraints(self):
        return len(self.dist_constraints) + 3 * len(self.angle_constraints)     # n_dof_lost (constraints.jl:358-372)


class VirtualSite:
    """VirtualSite (virtual.jl:10-22) with 0-based atom numbers (−1: unused): type 1/2/3/4 = OneParticleSite / TwoParticleAverageSite /
    ThreeParticleAverageSite / OutOfPlaneSite; weights that do not apply are zero; weight_cross in 1/nm."""
    __slots__ = ("type", "atom_ind", "atom_1", "atom_2", "atom_3", "weight_1", "weight_2", "weight_3", "weight_12", "weight_13", "weight_cross")

    def __init__(self, type, atom_ind, atom_1, atom_2=-1, atom_3=-1, weight_1=0.0, weight_2=0.0, weight_3=0.0, weight_12=0.0, weight_13=0.0, weight_cross=0.0):
        self.type, self.atom_ind, self.atom_1, self.atom_2, self.atom_3 = int(type), int(atom_ind), int(atom_1), int(atom_2), int(atom_3)
        self.weight_1, self.weight_2, self.weight_3 = float(weight_1), float(weight_2), float(weight_3)
        self.weight_12, self.weight_13, self.weight_cross = float(weight_12), float(weight_13), float(weight_cross)

    @property
    def weights(self):
        return (self.weight_1, self.weight_2, self.weight_3, self.weight_12, self.weight_13, self.weight_cross)


def _isapprox_one(x):
    return abs(x - 1.0) <= math.sqrt(np.finfo(np.float64).eps) * max(abs(x), 1.0)      # isapprox(x, 1), default rtol


def OneParticleSite(atom_ind, atom_1):
    """r = r₁ (virtual.jl:38-55)"""
    return VirtualSite(1, atom_ind, atom_1)


def TwoParticleAverageSite(atom_ind, atom_1, atom_2, weight_1, weight_2):
    """r = w₁ r₁ + w₂ r₂ with w₁ + w₂ = 1 (virtual.jl:57-76)"""
    if not _isapprox_one(weight_1 + weight_2):
        raise ValueError(f"weight_1 + weight_2 must equal 1 for a TwoParticleAverageSite, found {weight_1 + weight_2}")
    return VirtualSite(2, atom_ind, atom_1, atom_2, weight_1=weight_1, weight_2=weight_2)


def ThreeParticleAverageSite(atom_ind, atom_1, atom_2, atom_3, weight_1, weight_2, weight_3):
    """r = w₁ r₁ + w₂ r₂ + w₃ r₃ with w₁ + w₂ + w₃ = 1 (virtual.jl:78-98)"""
    if not _isapprox_one(weight_1 + weight_2 + weight_3):
        raise ValueError(f"weight_1 + weight_2 + weight_3 must equal 1 for a ThreeParticleAverageSite, found {weight_1 + weight_2 + weight_3}")
    return VirtualSite(3, atom_ind, atom_1, atom_2, atom_3, weight_1=weight_1, weight_2=weight_2, weight_3=weight_3)


def OutOfPlaneSite(atom_ind, atom_1, atom_2, atom_3, weight_12, weight_13, weight_cross):
    """r = r₁ + w₁₂ r₁₂ + w₁₃ r₁₃ + w_cross (r₁₂ × r₁₃) (virtual.jl:100-118); not compatible with the virial"""
    return VirtualSite(4, atom_ind, atom_1, atom_2, atom_3, weight_12=weight_12, weight_13=weight_13, weight_cross=weight_cross)


# ---- loggers (loggers.jl:131-283): what the engine's recorder takes inside the step loops (mhip_set_record), handed out as the reference's histories ----------
class _Logger:
    """a logger of the reference: records every n_steps steps (step_n % n_steps == 0, loggers.jl:98), values(logger) is its history; .steps are the step numbers"""
    channels = ()

    def __init__(self, n_steps):
        if int(n_steps) != n_steps or int(n_steps) < 1:
            raise ValueError(f"{type(self).__name__}: n_steps must be a positive integer, found {n_steps!r}")
        self.n_steps = int(n_steps)
        self.history = []
        self.steps = []

    def _value(self, rec, sys):
        raise NotImplementedError


class KineticEnergyLogger(_Logger):
    """KineticEnergyLogger(n_steps) (loggers.jl:146-168)"""
    channels = (_lib.REC_KE,)

    def _value(self, rec, sys):
        return rec[_lib.REC_KE]


class TemperatureLogger(_Logger):
    """TemperatureLogger(n_steps) (loggers.jl:131-144): 2·KE / (df·k) of the recorded kinetic energy (energy.jl:158-175)"""
    channels = (_lib.REC_KE,)

    def _value(self, rec, sys):
        return 2 * rec[_lib.REC_KE] / (_df(sys) * BOLTZMANN)


class PotentialEnergyLogger(_Logger):
    """PotentialEnergyLogger(n_steps) (loggers.jl:170-192): pairwise + specific + general"""
    channels = (_lib.REC_PE,)

    def _value(self, rec, sys):
        return _pe_total(rec[_lib.REC_PE])


class TotalEnergyLogger(_Logger):
    """TotalEnergyLogger(n_steps) (loggers.jl:194-214): kinetic + potential"""
    channels = (_lib.REC_KE, _lib.REC_PE)

    def _value(self, rec, sys):
        return rec[_lib.REC_KE] + _pe_total(rec[_lib.REC_PE])


class CoordinatesLogger(_Logger):
    """CoordinatesLogger(n_steps) (loggers.jl:216-250): one (n, 3) array per record"""
    channels = (_lib.REC_COORDS,)

    def _value(self, rec, sys):
        return rec[_lib.REC_COORDS]


class VelocitiesLogger(_Logger):
    """VelocitiesLogger(n_steps) (loggers.jl:252-283)"""
    channels = (_lib.REC_VELOCITIES,)

    def _value(self, rec, sys):
        return rec[_lib.REC_VELOCITIES]


def _pe_total(pe3):
    """the sum potential_energy() forms: pairwise, then specific, then general, starting from 0.0"""
    total = 0.0
    for x in pe3:
        total += float(x)
    return total


def values(logger):
    """values(logger) (loggers.jl:85)"""
    return logger.history


def _check_run_loggers(run_loggers):
    if not any(run_loggers is v for v in (True, False)) and run_loggers != "skipstart":      # loggers.jl:47-49
        raise ValueError(f"run_loggers must be True, False or 'skipstart', found {run_loggers!r}")
    return run_loggers


def _record_plan(loggers, init_step, n_steps, run_loggers=True):
    """What simulate() asks of the recorder for the steps init_step + 1 … init_step + n_steps: per channel the interval (the gcd of the n_steps of the loggers that
    need it, 0: off) and the capacity (the multiples of the interval in that range, and one more where the initial apply_loggers! records it), and the mask of
    that initial record (loggers.jl:50: always with True, with 'skipstart' only when init_step != 0; a logger records it when init_step % n_steps == 0)."""
    _check_run_loggers(run_loggers)
    every, capacity, start_mask = [0] * 4, [0] * 4, 0
    if run_loggers is False:
        return every, capacity, start_mask
    at_start = run_loggers is True or init_step != 0
    for lg in loggers:
        for c in lg.channels:
            every[c] = math.gcd(every[c], lg.n_steps)
            if at_start and init_step % lg.n_steps == 0:
                start_mask |= 1 << c
    for c in range(4):
        if every[c]:
            capacity[c] = (init_step + n_steps) // every[c] - init_step // every[c] + ((start_mask >> c) & 1)
            capacity[c] = max(capacity[c], 1)      # (a channel that is on needs room for one record)
    return every, capacity, start_mask


def _rng(rng):
    return rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)


def _rand_u64(rng):
    return int(rng.integers(0, 2 ** 64, dtype=np.uint64))          # rand(rng, UInt64)


# ---- System --------------------------------------------------------------------------------------------
class System:
    """System(; atoms, coords, boundary, velocities, pairwise_inters, specific_inter_lists, neighbor_finder)
    with array type "MI355X": every force/energy/integration call runs in libmollyhip.so."""

    def __init__(self, atoms=None, coords=None, boundary=None, velocities=None, pairwise_inters=(),
                 specific_inter_lists=(), neighbor_finder=None, dtype=np.float32, device_id=0,
                 charge=None, sigma=None, eps=None, mass=None, general_inters=(), lam=None, constraints=(), virtual_sites=(), loggers=None):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError("dtype must be float32 or float64")
        T = self.dtype
        if coords is None or boundary is None:
            raise ValueError("coords and boundary are required")
        self.coords = np.ascontiguousarray(coords, dtype=T).reshape(-1, 3).copy()
        n = len(self.coords)
        if atoms is not None:
            if len(atoms) != n:   # types.jl:914-916
                raise ValueError(f"there are {len(atoms)} atoms but {n} coordinates")
            charge = [a.charge for a in atoms]; sigma = [a.σ for a in atoms]; eps = [a.ϵ for a in atoms]
            mass = [a.mass for a in atoms]; lam = [a.λ for a in atoms]
            self.λ = np.ascontiguousarray(lam, dtype=T)
        else:
            self.λ = None if lam is None else np.ascontiguousarray(lam, dtype=T).reshape(n)      # (plain-array form of Atom.λ)
        arr = lambda a, d: np.full(n, d, T) if a is None else np.ascontiguousarray(a, dtype=T).reshape(n)
        self.charge, self.σ, self.ϵ, self.masses = arr(charge, 0), arr(sigma, 0), arr(eps, 0), arr(mass, 1)
        if velocities is not None and len(velocities) != n:
            raise ValueError(f"there are {n} coordinates but {len(velocities)} velocities")
        self.velocities = np.zeros((n, 3), T) if velocities is None else np.ascontiguousarray(velocities, dtype=T).reshape(n, 3).copy()
        self._ctx = None
        self._box_dirty = False
        self.boundary = boundary
        self.pairwise_inters = tuple(pairwise_inters)
        self.specific_inter_lists = tuple(specific_inter_lists)
        self.general_inters = tuple(general_inters)
        self.neighbor_finder = neighbor_finder if neighbor_finder is not None else NoNeighborFinder()
        self.device_id = device_id
        self.constraints = tuple(constraints)
        for c in self.constraints:
            if not isinstance(c, SHAKE_RATTLE):
                raise MollyHipError(-6, f"constraint algorithm {type(c).__name__} is outside the hot-path scope")
        if len(self.constraints) > 1:
            raise MollyHipError(-6, "one SHAKE_RATTLE per System")
        self.virtual_sites = tuple(virtual_sites)
        self.virtual_site_flags = np.zeros(n, bool)       # setup_virtual_sites (virtual.jl:120-180); the engine repeats these checks and adds its own
        for vi, vs in enumerate(self.virtual_sites):
            if not isinstance(vs, VirtualSite) or vs.type not in (1, 2, 3, 4):
                raise ValueError(f"unrecognised virtual site {vi}: type should be 1/2/3/4")
            if not 0 <= vs.atom_ind < n:
                raise ValueError(f"virtual site {vi} defines atom number {vs.atom_ind} but there are only {n} atoms present")
            if self.virtual_site_flags[vs.atom_ind]:
                raise ValueError(f"virtual site {vi} defines atom number {vs.atom_ind} but a previous virtual site already defined this atom")
            self.virtual_site_flags[vs.atom_ind] = True
        for vi, vs in enumerate(self.virtual_sites):
            for a in (vs.atom_1, vs.atom_2, vs.atom_3)[:(1, 2, 3, 3)[vs.type - 1]]:
                if not 0 <= a < n:
                    raise ValueError(f"virtual site {vi} has a parent atom out of range")
                if self.virtual_site_flags[a]:
                    raise ValueError(f"virtual site {vi} is defined in terms of an atom that is itself a virtual site")
        for sr in self.constraints:
            for c in list(sr.dist_constraints) + list(sr.angle_constraints):
                for a in (c.i, c.j) + ((c.k,) if hasattr(c, "k") else ()):
                    if 0 <= a < n and self.virtual_site_flags[a]:
                        raise ValueError(f"atom {a} is a virtual site but is also in a constraint")
        self.total_mass = float(self.masses.sum(dtype=np.float64))
        self._pushed_atoms = False
        self.loggers = dict(loggers) if loggers else {}      # name -> logger (types.jl:798-800); simulate() fills their histories from the engine's recorder
        for name, lg in self.loggers.items():
            if not isinstance(lg, _Logger):
                raise MollyHipError(-6, f"logger {name!r} ({type(lg).__name__}) is outside the hot-path scope: the engine records kinetic and potential "
                                        "energies, coordinates and velocities")

    def __len__(self):
        return len(self.coords)

    # `sys.boundary = …` on a live system (scale_coords!, spatial.jl:1202; the barostats' rejected moves, coupling.jl:930): the reference reads
    # sys.boundary at every force / energy call, so the engine's context follows the assignment (mhip_set_box) the next time state is pushed
    @property
    def boundary(self):
        return self._boundary

    @boundary.setter
    def boundary(self, b):
        b = b if isinstance(b, (CubicBoundary, TriclinicBoundary)) else CubicBoundary(b)
        old = getattr(self, "_boundary", None)
        if self._ctx is not None and old is not None:
            if type(b) is not type(old) or (isinstance(b, TriclinicBoundary) and b.approx_images != old.approx_images):
                raise MollyHipError(-6, "a live System keeps its kind of boundary (CubicBoundary / TriclinicBoundary and its image mode)")
            self._box_dirty = True
        self._boundary = b

    def _push_box(self):
        if not self._box_dirty or self._ctx is None:
            return
        b = self._boundary
        box = np.ascontiguousarray(b.side_lengths, dtype=np.float64)
        bv = np.ascontiguousarray(b.basis_vectors, dtype=np.float64) if isinstance(b, TriclinicBoundary) else None
        self._check(_lib.lib().mhip_set_box(self._ctx, self._ptr(box), self._ptr(bv)))
        self._box_dirty = False

    # -- interaction tuple → mhip_interactions ------------------------------------------------------------
    def interactions(self):
        it = _lib.Interactions()
        it.lj_weight_special = 1.0; it.coul_weight_special = 1.0; it.coul_ke = COULOMB_CONST; it.rf_dielectric = 1.0
        it.ewald_approx_erfc = 1
        n_coul = 0
        for inter in self.pairwise_inters:
            if isinstance(inter, LennardJones):
                if it.lj_enabled:
                    raise ValueError("only one LennardJones interaction is supported per System")
                it.lj_enabled = 1; it.lj_cutoff_kind = inter.cutoff.kind
                it.lj_rc = inter.cutoff.dist_cutoff; it.lj_ra = inter.cutoff.dist_activation
                it.lj_weight_special = inter.weight_special
            elif isinstance(inter, Coulomb):
                n_coul += 1
                it.coul_kind = _lib.COUL_PLAIN; it.coul_cutoff_kind = inter.cutoff.kind
                it.coul_rc = inter.cutoff.dist_cutoff; it.coul_ra = inter.cutoff.dist_activation
                it.coul_ke = inter.coulomb_const; it.coul_weight_special = inter.weight_special
            elif isinstance(inter, CoulombReactionField):
                n_coul += 1
                it.coul_kind = _lib.COUL_REACTION_FIELD; it.coul_rc = inter.dist_cutoff
                it.rf_dielectric = inter.solvent_dielectric; it.coul_ke = inter.coulomb_const
                it.coul_weight_special = inter.weight_special
            elif isinstance(inter, CoulombEwald):
                n_coul += 1
                it.coul_kind = _lib.COUL_EWALD_DIRECT; it.coul_rc = inter.dist_cutoff; it.ewald_alpha = inter.α
                it.ewald_approx_erfc = int(inter.approximate_erfc); it.coul_ke = inter.coulomb_const
                it.coul_weight_special = inter.weight_special
            else:
                raise MollyHipError(-6, f"pairwise interaction {type(inter).__name__} is outside the hot-path scope")
        if n_coul > 1:
            raise ValueError("only one Coulomb-type interaction is supported per System")
        return it

    def _uses_list(self):
        inters = self.pairwise_inters
        return any(use_neighbors(i) for i in inters) and math.isfinite(self.neighbor_finder.dist_cutoff)

    # -- engine context ----------------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise MollyHipError(rc, _lib.lib().mhip_last_error(self._ctx).decode())

    def engine(self):
        if self._ctx is not None:
            return self._ctx
        L = _lib.lib()
        inters = self.pairwise_inters
        if inters and len({bool(use_neighbors(i)) for i in inters}) > 1:
            raise MollyHipError(-6, "mixing use_neighbors=true and false interactions is not supported")
        cfg = _lib.Config()
        cfg.precision = 32 if self.dtype == np.float32 else 64
        cfg.device_id = self.device_id
        cfg.n_atoms = len(self)
        for d in range(3):
            cfg.box[d] = self.boundary.side_lengths[d]; cfg.origin[d] = 0.0; cfg.periodic[d] = 1
        cfg.rebuild_every = self.neighbor_finder.n_steps
        cfg.r_list = self.neighbor_finder.dist_cutoff if self._uses_list() else math.inf
        cfg.inter = self.interactions()
        ctx = C.c_void_p()
        rc = L.mhip_create(C.byref(ctx), C.byref(cfg))
        if rc != 0:
            raise MollyHipError(rc, L.mhip_last_error(None).decode())
        self._ctx = ctx
        if isinstance(self.boundary, TriclinicBoundary):
            bv = np.ascontiguousarray(self.boundary.basis_vectors, dtype=np.float64)
            self._check(L.mhip_set_triclinic(ctx, self._ptr(bv), 1 if self.boundary.approx_images else 0))
        self._push_atoms()
        return ctx

    def _ptr(self, a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def _push_atoms(self):
        L = _lib.lib()
        self._check(L.mhip_set_atoms(self._ctx, self._ptr(self.charge), self._ptr(self.σ), self._ptr(self.ϵ),
                                     self._ptr(self.masses), self._ptr(self.λ), _lib.MEM_HOST))
        nf = self.neighbor_finder
        if self._uses_list() or len(nf.excluded) or len(nf.special):
            ex = np.ascontiguousarray(nf.excluded, dtype=np.int32).reshape(-1, 2)
            sp = np.ascontiguousarray(nf.special, dtype=np.int32).reshape(-1, 2)
            exi, exj = np.ascontiguousarray(ex[:, 0]), np.ascontiguousarray(ex[:, 1])
            spi, spj = np.ascontiguousarray(sp[:, 0]), np.ascontiguousarray(sp[:, 1])
            self._check(L.mhip_set_exceptions(self._ctx, self._ptr(exi), self._ptr(exj), len(exi), self._ptr(spi), self._ptr(spj), len(spi)))
        T = self.dtype
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        f = lambda a: np.ascontiguousarray(a, dtype=T)
        for sil in self.specific_inter_lists:
            if isinstance(sil, HarmonicBonds):
                a = [i32(sil.i), i32(sil.j), f(sil.k), f(sil.r0)]
                self._check(L.mhip_set_bonds(self._ctx, len(a[0]), *map(self._ptr, a)))
            elif isinstance(sil, HarmonicAngles):
                a = [i32(sil.i), i32(sil.j), i32(sil.k), f(sil.kθ), f(sil.θ0)]
                self._check(L.mhip_set_angles(self._ctx, len(a[0]), *map(self._ptr, a)))
            elif isinstance(sil, PeriodicTorsions):
                a = [i32(sil.i), i32(sil.j), i32(sil.k), i32(sil.l), i32(sil.periodicity), f(sil.phase), f(sil.k0)]
                self._check(L.mhip_set_torsions(self._ctx, len(a[0]), *map(self._ptr, a)))
            elif isinstance(sil, EwaldExclusions):
                a = [i32(sil.i), i32(sil.j)]
                self._check(L.mhip_set_ewald_exclusions(self._ctx, len(a[0]), *map(self._ptr, a)))
            else:
                raise MollyHipError(-6, f"specific interaction list {type(sil).__name__} is outside the hot-path scope")
        for gi in self.general_inters:
            if isinstance(gi, PME):
                mesh = (C.c_int32 * 3)(*gi.mesh_dims)
                self._check(L.mhip_set_pme(self._ctx, gi.order, mesh, gi.α, gi.ϵr))
            else:
                raise MollyHipError(-6, f"general interaction {type(gi).__name__} is outside the hot-path scope")
        for sr in self.constraints:
            dc, ac = sr.dist_constraints, sr.angle_constraints
            ci, cj = i32([c.i for c in dc]), i32([c.j for c in dc])
            cd = np.ascontiguousarray([c.dist for c in dc], dtype=np.float64)
            ai, aj, ak = i32([c.i for c in ac]), i32([c.j for c in ac]), i32([c.k for c in ac])
            d3 = np.ascontiguousarray([(c.dist_ij, c.dist_jk, c.dist_ik) for c in ac], dtype=np.float64).reshape(-1)
            self._check(L.mhip_set_constraints(self._ctx, len(ci), *map(self._ptr, (ci, cj, cd)), len(ai), *map(self._ptr, (ai, aj, ak, d3)),
                                               sr.dist_tolerance, sr.vel_tolerance, sr.max_iters))

        if self.virtual_sites:
            vs = self.virtual_sites
            cols = [i32([getattr(v, k) for v in vs]) for k in ("type", "atom_ind", "atom_1", "atom_2", "atom_3")]
            w6 = np.ascontiguousarray([v.weights for v in vs], dtype=np.float64).reshape(-1)
            self._check(L.mhip_set_virtual_sites(self._ctx, len(vs), *map(self._ptr, cols), self._ptr(w6)))

    @property
    def n_constraints(self):
        return sum(c.n_constraints for c in self.constraints)

    def virtual_site_info(self):
        """mhip_virtual_site_info: sites of each type, sites hosted by a work item of the step loops, items that host one, unconstrained groups formed"""
        out = (C.c_int64 * 8)()
        self._check(_lib.lib().mhip_virtual_site_info(self.engine(), C.byref(out)))
        keys = ("one_particle", "two_particle", "three_particle", "out_of_plane", "n_hosted", "n_host_items", "n_groups")
        return dict(zip(keys, list(out)[:7]))

    def _refuse_sites(self, what):
        if self.virtual_sites:
            raise MollyHipError(-6, f"{what} of a System with virtual sites is not supported")

    def constraint_info(self):
        """mhip_constraint_info: clusters of 2 / 3 / 4 atoms, angle clusters, constraints, the most SHAKE iterations of the last run,
        cluster-solves stopped at max_iters since the constraints were set"""
        out = (C.c_int64 * 8)()
        self._check(_lib.lib().mhip_constraint_info(self.engine(), C.byref(out)))
        keys = ("clusters12", "clusters23", "clusters34", "angle_clusters", "n_constraints", "max_iters_last_run", "n_not_converged")
        return dict(zip(keys, list(out)[:7]))

    def thermostat_info(self):
        """mhip_thermostat_info: what the rescaling thermostat of the last coupled simulate did (written on the device, read with the run's end)"""
        out = (C.c_double * 8)()
        self._check(_lib.lib().mhip_thermostat_info(self.engine(), out))
        keys = ("n_applied", "last_step", "last_lambda", "last_kinetic_energy", "min_lambda", "max_lambda", "n_refused")
        return dict(zip(keys, list(out)[:7]))

    def _refuse_constrained(self, what):
        if self.constraints:
            raise MollyHipError(-6, f"{what} of a constrained System is not supported (the rigid-molecule treatment stays in Julia)")

    def push_state(self, velocities=True):
        L = _lib.lib()
        self.engine()
        self._push_box()
        self._check(L.mhip_set_state(self._ctx, self._ptr(self.coords), self._ptr(self.velocities) if velocities else None, _lib.MEM_HOST))

    def pull_state(self):
        L = _lib.lib()
        self._check(L.mhip_get_state(self._ctx, self._ptr(self.coords), self._ptr(self.velocities), _lib.MEM_HOST))

    def stats(self):
        st = _lib.Stats()
        self._check(_lib.lib().mhip_get_stats(self.engine(), C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._ctx is not None:
            _lib.lib().mhip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- free functions mirroring Molly's exports ---------------------------------------------------------
def forces(sys, step_n=0, pairwise=True, specific=True, general=True):
    """forces(sys; …): pairwise + specific + general interaction forces, (n,3) array (force.jl:670-720, 792-795)."""
    L = _lib.lib()
    sys.push_state(velocities=False)
    out = np.zeros((len(sys), 3), sys.dtype)
    if pairwise and sys.pairwise_inters:
        sys._check(L.mhip_forces(sys._ctx, step_n, 1, sys._ptr(out), None, _lib.MEM_HOST))
    if specific and sys.specific_inter_lists:
        sys._check(L.mhip_specific_forces(sys._ctx, 1, sys._ptr(out), _lib.MEM_HOST))
    if general and sys.general_inters:
        sys._check(L.mhip_general_forces(sys._ctx, 1, sys._ptr(out), _lib.MEM_HOST))
    if sys.virtual_sites:                                         # distribute_forces! on the total (force.jl:796)
        sys._check(L.mhip_distribute_forces(sys._ctx, sys._ptr(out), _lib.MEM_HOST))
    return out


def place_virtual_sites(sys):
    """place_virtual_sites!(sys) (virtual.jl:187-224): the sites' coordinates from their parents', on the device"""
    if sys.virtual_sites:
        sys.push_state(velocities=True)
        sys._check(_lib.lib().mhip_place_virtual_sites(sys._ctx))
        sys.pull_state()
    return sys


_forces_of = forces      # (constraint_virial takes an argument of that name)


def constraint_virial(sys, forces=None, dt=0.0005, parts=False):
    """The constraint contribution to the virial at the current coordinates and velocities, 3×3, by the reference's trial step
    (merge_initial_constraint_virial!, simulators.jl:459-495; per-cluster accumulation shake.jl:234-392): RATTLE, a kick by dt and RATTLE, a drift by dt
    and SHAKE, all on the device in double precision (mhip_constraint_virial); the System is left as it was.  forces: the total forces, (n, 3), virtual-site
    rows distributed (None: forces(sys)).  dt [ps]: the preview step, the reference's 0.0005 by default — the result depends on it at first order.
    parts=True: (W, Wv, Wp), the RATTLE and the SHAKE part.  Zeros without constraints."""
    if not (isinstance(dt, (int, float, np.floating)) and math.isfinite(dt) and dt > 0):
        raise ValueError("dt must be positive and finite")
    n = len(sys)
    if forces is not None:
        forces = np.ascontiguousarray(forces, dtype=sys.dtype)
        if forces.shape != (n, 3):
            raise ValueError(f"forces must have the shape ({n}, 3), not {forces.shape}")
    w = np.zeros(9, np.float64); p18 = np.zeros(18, np.float64)
    if sys.constraints:
        if forces is None:
            forces = _forces_of(sys)
        sys.push_state(velocities=True)
        bad = C.c_int64(0)
        sys._check(_lib.lib().mhip_constraint_virial(sys._ctx, sys._ptr(forces), _lib.MEM_HOST, float(dt), w.ctypes.data_as(C.c_void_p),
                                                     p18.ctypes.data_as(C.c_void_p), C.byref(bad)))
        if bad.value:
            warnings.warn(f"constraint_virial: {bad.value} cluster solves stopped at max_iters")
    w = w.reshape(3, 3)
    return (w, p18[:9].reshape(3, 3), p18[9:].reshape(3, 3)) if parts else w


def virial(sys, step_n=0, pairwise=True, specific=True, general=True, constraints=False):
    """virial(sys): 3×3 tensor Σ r ⊗ f of the pairwise (over the neighbour pairs, force.jl:848-852), specific (force.jl:991-1060) and
    general (PME reciprocal space, ewald.jl:701-723, 925-927) interactions (energy.jl:116-131).
    constraints=True adds constraint_virial(sys) (the reference's virial(sys) always does, compute_initial_total_virial!, simulators.jl:529-536); a
    constrained System is refused without it, as it has been.  Making the term the default is a later, separate change of behaviour."""
    if not constraints:
        sys._refuse_constrained("virial")
    if any(vs.type == 4 for vs in sys.virtual_sites):
        raise MollyHipError(-6, "OutOfPlaneSite is not currently compatible with virial calculation (virtual.jl:112)")
    L = _lib.lib()
    sys.push_state(velocities=False)
    v = np.zeros(9, np.float64)
    vp = v.ctypes.data_as(C.c_void_p)
    if pairwise and sys.pairwise_inters:
        out = np.zeros((len(sys), 3), sys.dtype)
        sys._check(L.mhip_forces(sys._ctx, step_n, 0, sys._ptr(out), vp, _lib.MEM_HOST))
    if specific and sys.specific_inter_lists:
        sys._check(L.mhip_specific_virial(sys._ctx, vp))
    if general and sys.general_inters:
        sys._check(L.mhip_general_virial(sys._ctx, vp))
    v = v.reshape(3, 3)
    if constraints and sys.constraints:
        v = v + constraint_virial(sys, forces(sys, step_n))
    return v


def scalar_virial(sys, step_n=0, constraints=False):
    """scalar_virial(sys) = tr(virial(sys)) (energy.jl:148-151)"""
    return float(np.trace(virial(sys, step_n, constraints=constraints)))


def pressure(sys, step_n=0, constraints=False):
    """pressure(sys) = (2K + W) / V with K = ½ Σ m v ⊗ v (spatial.jl:930-982), in kJ mol⁻¹ nm⁻³ (1 kJ mol⁻¹ nm⁻³ = 16.6054 bar); constraints: as virial's"""
    w = virial(sys, step_n, constraints=constraints)
    v = np.asarray(sys.velocities, dtype=np.float64); m = np.asarray(sys.masses, dtype=np.float64)
    k = 0.5 * np.einsum("i,ia,ib->ab", m, v, v)
    return (2.0 * k + w) / float(np.prod(sys.boundary.side_lengths))


def scalar_pressure(sys, step_n=0, constraints=False):
    return float(np.trace(pressure(sys, step_n, constraints=constraints))) / 3.0


def potential_energy(sys, step_n=0, pairwise=True, specific=True, general=True):
    """potential_energy(sys; …) (energy.jl:207-248, 409-446)."""
    L = _lib.lib()
    sys.push_state(velocities=False)
    total = 0.0
    pe = C.c_double(0)
    if pairwise and sys.pairwise_inters:
        sys._check(L.mhip_potential_energy(sys._ctx, step_n, C.byref(pe)))
        total += pe.value
    if specific and sys.specific_inter_lists:
        sys._check(L.mhip_specific_potential_energy(sys._ctx, C.byref(pe)))
        total += pe.value
    if general and sys.general_inters:
        sys._check(L.mhip_general_potential_energy(sys._ctx, C.byref(pe)))
        total += pe.value
    return total


def kinetic_energy(sys):
    L = _lib.lib()
    sys.push_state(velocities=True)
    ke = C.c_double(0)
    sys._check(L.mhip_kinetic_energy(sys._ctx, C.byref(ke)))
    return ke.value


def _df(sys):
    """sys.df = 3(N − n_sites) − 3 − n_constraints for a fully periodic box (constraints.jl:358-380, types.jl:957-959)"""
    return 3 * (len(sys) - len(sys.virtual_sites)) - 3 - sys.n_constraints


def temperature(sys):
    """T = 2 KE / (df k) (energy.jl:158-175)."""
    return 2 * kinetic_energy(sys) / (_df(sys) * BOLTZMANN)


def total_energy(sys):
    return kinetic_energy(sys) + potential_energy(sys)


def find_neighbors(sys, step_n=0):
    """find_neighbors(sys, sys.neighbor_finder) → NeighborList (neighbors.jl:390-423); None without a list."""
    if not sys._uses_list():
        return None
    L = _lib.lib()
    sys.push_state(velocities=False)
    sys._check(L.mhip_rebuild(sys._ctx, step_n))
    n = C.c_int64(0)
    sys._check(L.mhip_export_neighbors(sys._ctx, None, None, None, 0, C.byref(n)))
    i = np.empty(n.value, np.int32); j = np.empty(n.value, np.int32); sp = np.empty(n.value, np.uint8)
    if n.value:
        sys._check(L.mhip_export_neighbors(sys._ctx, sys._ptr(i), sys._ptr(j), sys._ptr(sp), n.value, C.byref(n)))
    return NeighborList(i, j, sp)


def optimize_launch_config(sys, n_passes=20):
    """optimize_cuda_launch_config!(sys) (src/cuda_config.jl:53-62, ext/MollyCUDAExt.jl:594-642): time the candidate workgroup shapes of the
    search / pair kernels on this system, keep the fastest; returns [(block_atoms, j_split, µs per force pass), …] (µs < 0: not launchable)."""
    L = _lib.lib()
    sys.push_state(velocities=False)
    tr = (_lib.LaunchTrial * 16)()
    n = C.c_int32(0)
    sys._check(L.mhip_optimize_launch_config(sys.engine(), int(n_passes), tr, 16, C.byref(n)))
    return [(t.block_atoms, t.j_split, float(t.us_per_pass)) for t in tr[: min(n.value, 16)]]


def set_launch_config(sys, block_atoms=0, j_split=0):
    """set_cuda_launch_config!(sys; …) / reset_cuda_launch_config!(sys) with the defaults (src/cuda_config.jl:17-47)."""
    sys._check(_lib.lib().mhip_set_launch_config(sys.engine(), int(block_atoms), int(j_split)))


def remove_CM_motion(sys):
    """remove_CM_motion!(sys) (spatial.jl:901-929)."""
    L = _lib.lib()
    sys.push_state(velocities=True)
    sys._check(L.mhip_remove_cm(sys._ctx))
    sys.pull_state()
    return sys


def _minimize(sys, sim, init_step=0):
    """simulate!(sys, ::SteepestDescentMinimizer) (simulators.jl:183-271; systems without constraints or virtual sites): every force and energy from the engine, the
    update x += hn · F / max|F| and the accept / reject rule in the system's number type on the host side, as the reference's loop broadcasts them"""
    T = sys.dtype.type
    log = (lambda *a: print(*a, file=sim.log_stream)) if sim.log_stream is not None else (lambda *a: None)
    sys.coords[:] = wrap_coords(sys.coords, sys.boundary)
    E = potential_energy(sys, init_step)
    log("Step", init_step, "- potential energy", E, "- max force N/A - N/A")
    hn = T(sim.step_size)
    for step_n in range(init_step + 1, init_step + sim.max_steps + 1):
        F = forces(sys, step_n)
        max_force = np.sqrt((F * F).sum(axis=1, dtype=sys.dtype)).max()               # maximum(norm.(F))
        coords_copy = sys.coords.copy()
        sys.coords[:] = wrap_coords(sys.coords + (hn * F / max_force).astype(sys.dtype), sys.boundary)
        E_trial = potential_energy(sys, step_n)
        if E_trial < E:
            hn = T(6) * hn / T(5)
            E = E_trial
            log("Step", step_n, "- potential energy", E_trial, "- max force", max_force, "- accepted")
        else:
            sys.coords[:] = coords_copy
            hn = hn / T(5)
            log("Step", step_n, "- potential energy", E_trial, "- max force", max_force, "- rejected")
        if max_force < sim.tol:
            break
    return sys


def _minimize_engine(sys, sim, init_step=0):
    """The same loop inside the engine (mhip_minimize): the state goes over once and comes back once, the log lines are printed from the call's records"""
    k = 0.0 if sim.constraint_bond_constant is None else float(sim.constraint_bond_constant)
    n = int(sim.max_steps)
    log4 = np.zeros((max(n, 1), 4), np.float64); out8 = np.zeros(8, np.float64)
    sys.push_state(velocities=True)
    sys._check(_lib.lib().mhip_minimize(sys._ctx, int(init_step), n, float(sim.step_size), float(sim.tol), k,
                                        log4.ctypes.data_as(C.POINTER(C.c_double)), out8.ctypes.data_as(C.POINTER(C.c_double))))
    sys.pull_state()
    if sim.log_stream is not None:
        print("Step", init_step, "- potential energy", out8[0], "- max force N/A - N/A", file=sim.log_stream)
        for s in range(int(out8[4])):
            print("Step", init_step + 1 + s, "- potential energy", log4[s, 0], "- max force", sys.dtype.type(log4[s, 1]), "-", "accepted" if log4[s, 2] else "rejected", file=sim.log_stream)
    return sys


def _read_records(sys, L, every, replaced):
    """the recorder's history, read once: per channel {step: value}; replaced: {(channel, step): value} taken on the host side (a barostat's move behind a record)"""
    T = sys.dtype
    info = (C.c_int64 * 16)()
    sys._check(L.mhip_record_info(sys._ctx, C.byref(info)))
    out = {}
    for c in range(4):
        if not every[c]:
            continue
        n = int(info[4 * c + 2])
        steps = np.zeros(n, np.int64)
        shape = {_lib.REC_KE: (n,), _lib.REC_PE: (n, 3)}.get(c, (n, len(sys), 3))
        vals = np.zeros(shape, T if c >= _lib.REC_COORDS else np.float64)
        if n:
            sys._check(L.mhip_record_read(sys._ctx, c, 0, n, sys._ptr(steps), sys._ptr(vals), _lib.MEM_HOST))
        vals = vals.tolist() if c == _lib.REC_KE else vals      # (python floats for the scalar channel: the histories hold what kinetic_energy() returns)
        out[c] = {int(s): replaced.get((c, int(s)), vals[k]) for k, s in enumerate(steps)}
    return out


def _fill_loggers(sys, records):
    """append to each logger the records whose step is a multiple of its own n_steps (loggers.jl:98), in step order"""
    for lg in sys.loggers.values():
        for s in sorted(records[lg.channels[0]]):
            if s % lg.n_steps == 0 and all(s in records[c] for c in lg.channels):
                v = lg._value({c: records[c][s] for c in lg.channels}, sys)
                lg.history.append(v.copy() if isinstance(v, np.ndarray) else v)
                lg.steps.append(s)


def simulate(sys, sim, n_steps=None, init_step=0, check_nans=False, rng=None, run_loggers=True):
    """simulate!(sys, sim, n_steps; init_step, rng) for VelocityVerlet (simulators.jl:547-668), Langevin (:1099-1220), LangevinSplitting (:1255-1381, coupling
    nothing or AndersenThermostat) and OverdampedLangevin (:1426-1489); the first two with
    coupling nothing, AndersenThermostat, MonteCarloBarostat or a tuple of the two; VelocityVerlet also takes ImmediateThermostat, BerendsenThermostat and
    VelocityRescaleThermostat (alone or with the barostat), applied inside the device loop.  The step loop runs on the device; with a barostat it is cut at the
    multiples of barostat.n_steps, where apply_coupling! runs on the host side of the boundary with the engine's potential energies (the README's GPU
    example: Langevin + MonteCarloBarostat).  Coordinates and velocities come back when the call returns.  rng: a numpy Generator or a seed; as in the
    reference it supplies the Philox key / counter words and the barostat's uniform numbers.
    sys.loggers (apply_loggers!, loggers.jl:44-56; run_loggers True, False or "skipstart"): VelocityVerlet and Langevin record inside the device loop — the
    engine's recorder is set for the call (one interval per channel: the gcd of the loggers that need it), the initial record is taken, the run is made as
    without loggers, the channels are read once at the end and each logger gets the records at the multiples of its own n_steps.  A record at a step on which
    the barostat applies is taken again behind its move, as the reference logs behind apply_coupling!.  The other simulators refuse loggers."""
    _check_run_loggers(run_loggers)
    recording = bool(sys.loggers) and run_loggers is not False
    if recording and isinstance(sim, (SteepestDescentMinimizer, LangevinSplitting, OverdampedLangevin)):
        raise MollyHipError(-6, f"loggers are recorded inside the VelocityVerlet and Langevin loops only: {type(sim).__name__} does not record (run_loggers=False runs it without them)")
    if isinstance(sim, SteepestDescentMinimizer) and sim.engine_loop:
        if init_step < 0:
            raise ValueError("init_step must be non-negative")
        return _minimize_engine(sys, sim, init_step)
    if isinstance(sim, SteepestDescentMinimizer):
        sys._refuse_constrained("minimization")
        sys._refuse_sites("minimization")
        if init_step < 0:
            raise ValueError("init_step must be non-negative")
        return _minimize(sys, sim, init_step)
    if not isinstance(sim, (VelocityVerlet, Langevin, LangevinSplitting, OverdampedLangevin)):
        raise MollyHipError(-6, f"simulator {type(sim).__name__} is outside the hot-path scope")
    if n_steps is None:
        raise TypeError("simulate: n_steps is required for VelocityVerlet and Langevin")
    splitting = isinstance(sim, (LangevinSplitting, OverdampedLangevin))
    couplings = sim.coupling if isinstance(sim.coupling, (tuple, list)) else (() if sim.coupling is None else (sim.coupling,))
    thermostat = barostat = rescale = None
    for c in couplings:
        if isinstance(c, AndersenThermostat) and thermostat is None:
            thermostat = c
        elif type(c) in _RESCALE_KIND and rescale is None and not splitting:
            rescale = c
        elif isinstance(c, MonteCarloBarostat) and barostat is None and not splitting:
            barostat = c
        else:
            raise MollyHipError(-6, f"coupling {type(c).__name__} is outside the hot-path scope")
    if init_step < 0:   # check_simulate_inputs
        raise ValueError("init_step must be non-negative")
    if barostat is not None:
        sys._refuse_constrained("MonteCarloBarostat coupling")
        sys._refuse_sites("MonteCarloBarostat coupling")
    if rescale is not None and isinstance(sim, Langevin):
        raise MollyHipError(-6, f"{type(rescale).__name__} is a coupling of VelocityVerlet, not of Langevin")
    if rescale is not None and thermostat is not None:
        raise MollyHipError(-6, f"{type(rescale).__name__} next to AndersenThermostat is not supported")
    if thermostat is not None and sys.virtual_sites:
        raise MollyHipError(-6, "AndersenThermostat coupling of a System with virtual sites is not supported")
    if thermostat is not None and sys.constraints:
        raise MollyHipError(-6, "AndersenThermostat coupling of a constrained System is not supported")
    L = _lib.lib()
    rng = _rng(rng)
    sys.push_state(velocities=True)
    if thermostat is not None:
        sys._check(L.mhip_set_andersen(sys._ctx, BOLTZMANN * float(thermostat.temperature), float(sim.dt) / float(thermostat.coupling_const), _rand_u64(rng)))
    every, replaced = [0] * 4, {}
    try:
        if recording:
            every, capacity, start_mask = _record_plan(sys.loggers.values(), init_step, n_steps, run_loggers)
            sys._check(L.mhip_set_record(sys._ctx, C.byref((C.c_int32 * 4)(*every)), C.byref((C.c_int64 * 4)(*capacity))))
            if start_mask:                                         # the loggers before the first step (simulators.jl:571, 1120)
                sys._check(L.mhip_record_now(sys._ctx, init_step, start_mask))
        if rescale is not None:      # key and ctr1 once per call; application s draws from (key, ctr1 + s) on the device
            sys._check(L.mhip_set_thermostat(sys._ctx, _RESCALE_KIND[type(rescale)], BOLTZMANN * float(rescale.temperature), float(getattr(rescale, "coupling_const", 1.0)),
                                             int(getattr(rescale, "n_steps", 1)), _df(sys), _rand_u64(rng), _rand_u64(rng)))
        if isinstance(sim, Langevin):
            key, ctr1 = _rand_u64(rng), _rand_u64(rng)             # simulators.jl:1149-1150
        if isinstance(sim, LangevinSplitting):                     # key, then ctr1 (simulators.jl:1291-1292); a splitting without an O draws nothing
            key, ctr1 = (_rand_u64(rng), _rand_u64(rng)) if "O" in sim.splitting else (0, 0)
            sys._check(L.mhip_splitting_run(sys._ctx, init_step, n_steps, sim.dt, BOLTZMANN * sim.temperature, sim.friction, sim.splitting.encode(),
                                            int(sim.remove_CM_motion), key, ctr1))
        if isinstance(sim, OverdampedLangevin):                    # one key and a counter that advances per step (mollyhip.h)
            key, ctr1 = _rand_u64(rng), _rand_u64(rng)
            sys._check(L.mhip_overdamped_run(sys._ctx, init_step, n_steps, sim.dt, BOLTZMANN * sim.temperature, sim.friction, int(sim.remove_CM_motion), key, ctr1))
        first, last = init_step, init_step + (0 if splitting else n_steps)
        while first < last:
            nxt = last if barostat is None else min(last, (first // barostat.n_steps + 1) * barostat.n_steps)
            if isinstance(sim, Langevin):                         # ctr1 advances by one per step (simulators.jl:1190)
                sys._check(L.mhip_langevin_run(sys._ctx, first, nxt - first, sim.dt, BOLTZMANN * sim.temperature, sim.friction,
                                               int(sim.remove_CM_motion), key, (ctr1 + (first - init_step)) % 2 ** 64))
            else:
                sys._check(L.mhip_vv_run(sys._ctx, first, nxt - first, float(sim.dt), int(sim.remove_CM_motion)))
            if barostat is not None and nxt % barostat.n_steps == 0:      # apply_coupling! at the end of step nxt (simulators.jl:1192)
                sys.pull_state()
                _apply_mc_barostat(sys, barostat, nxt, rng)
                sys.push_state(velocities=True)                   # the accepted box and coordinates, or the old ones back after a rejected trial
                if every[_lib.REC_COORDS] and nxt % every[_lib.REC_COORDS] == 0:      # the loggers run behind the coupling (simulators.jl:630, 657)
                    replaced[(_lib.REC_COORDS, nxt)] = sys.coords.copy()
                if every[_lib.REC_PE] and nxt % every[_lib.REC_PE] == 0:
                    replaced[(_lib.REC_PE, nxt)] = [potential_energy(sys, nxt, pairwise=k == 0, specific=k == 1, general=k == 2) for k in range(3)]
            first = nxt
        if recording:
            _fill_loggers(sys, _read_records(sys, L, every, replaced))
    finally:
        if recording:
            sys._check(L.mhip_set_record(sys._ctx, C.byref((C.c_int32 * 4)()), C.byref((C.c_int64 * 4)())))
        if thermostat is not None:
            sys._check(L.mhip_set_andersen(sys._ctx, 0.0, 0.0, 0))
        if rescale is not None:
            sys._check(L.mhip_set_thermostat(sys._ctx, 0, 0.0, 0.0, 1, 0, 0, 0))
    if check_nans:
        sys._check(L.mhip_check_finite(sys._ctx))
    if sys.constraints and sys.constraint_info()["n_not_converged"] > 0:        # shake.jl:817
        sr = sys.constraints[0]
        warnings.warn(f"SHAKE did not converge within {sr.max_iters} iterations for some clusters ({sys.constraint_info()['n_not_converged']} "
                      "cluster-solves so far); consider a smaller time step or a larger max_iters")
    sys.pull_state()
    return sys


def random_velocities(sys, temp, rng=None):
    """random_velocities!(sys, temp; rng) (spatial.jl:803-831): Maxwell-Boltzmann velocities at temperature temp (K), drawn on the device"""
    L = _lib.lib()
    rng = _rng(rng)
    sys.push_state(velocities=True)
    ctr1, key = _rand_u64(rng), _rand_u64(rng)
    sys._check(L.mhip_random_velocities(sys._ctx, BOLTZMANN * float(temp), key, ctr1))
    sys.pull_state()
    return sys


def apply_coupling(sys, coupling, sim, rng=None, step_n=0):
    """apply_coupling!(sys, buffers, coupling, sim, neighbors, step_n; rng): one application.  AndersenThermostat (coupling.jl:196-211) returns False;
    MonteCarloBarostat (coupling.jl:861-1033) returns whether a move was accepted (the forces must be recomputed)."""
    if isinstance(coupling, MonteCarloBarostat):
        return _apply_mc_barostat(sys, coupling, step_n, _rng(rng))
    thermostat = coupling
    if not isinstance(thermostat, AndersenThermostat):
        raise MollyHipError(-6, f"coupling {type(thermostat).__name__} is outside the hot-path scope")
    L = _lib.lib()
    rng = _rng(rng)
    sys.push_state(velocities=True)
    ctr1, key = _rand_u64(rng), _rand_u64(rng)
    sys._check(L.mhip_andersen(sys._ctx, BOLTZMANN * float(thermostat.temperature), float(sim.dt) / float(thermostat.coupling_const), key, ctr1))
    sys.pull_state()
    return False


# ---- the boundary as a variable: what the barostats of coupling.jl need from the engine ---------------------------------------------------------------
BAR = 0.0602214076      # 1 bar in kJ mol⁻¹ nm⁻³ (1e5 Pa · 1e-27 m³/nm³ · N_A / 1e3)


def volume(boundary):
    """volume(boundary) (spatial.jl:365-372): the product of the side lengths; TriclinicBoundary: v1.x · v2.y · v3.z"""
    return float(np.prod(np.asarray(boundary.side_lengths, dtype=np.float64)))


def scale_boundary(boundary, scale):
    """scale_boundary(boundary, scale) (spatial.jl:414-422): a number or one factor per axis"""
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (3,))
    if isinstance(boundary, TriclinicBoundary):
        bv = boundary.basis_vectors
        return TriclinicBoundary(bv[0] * sc, bv[1] * sc, bv[2] * sc, approx_images=boundary.approx_images)
    return CubicBoundary(*(boundary.side_lengths * sc))


def scale_coords(sys, scale_matrix, scale_velocities=False):
    """scale_coords!(sys, μ; ignore_molecules=true) (spatial.jl:1184-1210, the branch of systems without a topology — every atom a molecule): box B′ = μ B,
    r′ = μ r in the system's number type, optionally v′ = μ⁻¹ v.  The rigid-molecule branch (:1211-1290) is host code on molecule lists and stays outside the
    engine; what the engine must do is follow the boundary (mhip_set_box)."""
    sys._refuse_sites("scale_coords")
    mu = np.asarray(scale_matrix, dtype=sys.dtype).reshape(3, 3)
    diagonal = not np.any(mu != np.diag(np.diag(mu)))
    b = sys.boundary
    if isinstance(b, TriclinicBoundary):
        nb = mu.astype(np.float64) @ b.basis_vectors.T            # columns = basis vectors (boxmatrix, spatial.jl:254)
        sys.boundary = TriclinicBoundary(nb[:, 0], nb[:, 1], nb[:, 2], approx_images=b.approx_images)
    else:
        if not diagonal:
            raise ValueError("a CubicBoundary is scaled by a diagonal matrix")
        sl = (np.diag(mu) * b.side_lengths.astype(sys.dtype)).astype(sys.dtype)   # μ · B in T, as the SMatrix product
        sys.boundary = CubicBoundary(*[float(x) for x in sl])
    sys.coords[:] = sys.coords * np.diag(mu)[None, :] if diagonal else (sys.coords @ mu.T).astype(sys.dtype)
    if scale_velocities:
        mi = np.linalg.inv(mu.astype(np.float64)).astype(sys.dtype)
        sys.velocities[:] = (sys.velocities @ mi.T).astype(sys.dtype)
    return sys


class MonteCarloBarostat:
    """MonteCarloBarostat(pressure, temperature, boundary; coupling_type=:isotropic, n_steps=30, n_iterations=1, scale_factor=0.01, scale_increment=1.1,
    max_volume_frac=0.3, trial_find_neighbors=false) (coupling.jl:721-859).  pressure in bar: a number (isotropic) or the three diagonal entries Pxx, Pyy, Pzz
    (semiisotropic, anisotropic).  The trial energies are full potential energies of the engine on the scaled box (the GPU path of the reference evaluates
    the cutoff sphere from the coordinates at every call, so `trial_find_neighbors` has nothing to choose there; it is kept for the signature)."""

    def __init__(self, pressure, temperature, boundary, coupling_type="isotropic", n_steps=30, n_iterations=1, scale_factor=0.01,
                 scale_increment=1.1, max_volume_frac=0.3, trial_find_neighbors=False):
        if coupling_type not in ("isotropic", "semiisotropic", "anisotropic"):      # coupling.jl:788-790
            raise ValueError("coupling_type must be :isotropic, :semiisotropic, or :anisotropic")
        p = np.asarray(pressure, dtype=np.float64)
        if coupling_type == "isotropic":
            if p.ndim != 0:
                raise ValueError("isotropic pressure must be a scalar")
            p = np.full(3, float(p))
        elif p.shape != (3,):
            raise ValueError(f"{coupling_type} pressure must have the three diagonal entries Pxx, Pyy, Pzz")
        self.pressure = p.copy()                                  # bar
        self.temperature = float(temperature)
        self.coupling_type = coupling_type
        self.n_steps, self.n_iterations = int(n_steps), int(n_iterations)
        self.volume_scale = volume(boundary) * float(scale_factor)
        self.scale_increment, self.max_volume_frac = float(scale_increment), float(max_volume_frac)
        self.trial_find_neighbors = bool(trial_find_neighbors)
        self.n_attempted = 0
        self.n_accepted = 0


def _mc_attempt(sys, barostat, E, rand, n_molecules):
    """one trial of apply_coupling_mc! (coupling.jl:886-1033) up to the trial state: scales sys, returns (dW-without-ΔE as a function of E_trial, undo)"""
    T = sys.dtype.type
    V = T(volume(sys.boundary))
    dV = T(barostat.volume_scale) * (T(2) * rand() - T(1))
    v_scale = (V + dV) / V
    kT = BOLTZMANN * barostat.temperature
    P = barostat.pressure * BAR
    if barostat.coupling_type == "isotropic":
        l = np.cbrt(v_scale)
        diag = (l, l, l)
        work = float(P.sum()) * float(dV) / 3.0                                   # tr(P) · dV / 3
    elif barostat.coupling_type == "semiisotropic":
        w1, w2 = rand(), rand()
        s_ = w1 + w2; w1, w2 = w1 / s_, w2 / s_
        lxy, lz = v_scale ** w1, v_scale ** w2
        diag = (lxy, lxy, lz)
        work = float((w1 / T(2)) * P[0] + (w1 / T(2)) * P[1] + w2 * P[2]) * float(V + dV) * math.log(float(v_scale))
    else:
        w1, w2, w3 = rand(), rand(), rand()
        s_ = w1 + w2 + w3; w1, w2, w3 = w1 / s_, w2 / s_, w3 / s_
        diag = (v_scale ** w1, v_scale ** w2, v_scale ** w3)
        work = float(w1 * P[0] + w2 * P[1] + w3 * P[2]) * float(V + dV) * math.log(float(v_scale))
    old_coords, old_boundary = sys.coords.copy(), sys.boundary
    scale_coords(sys, np.diag(np.asarray(diag, dtype=sys.dtype)))
    dW_of = lambda E_trial: (E_trial - E) + work - n_molecules * kT * math.log(float(v_scale))

    def undo():
        sys.coords[:] = old_coords
        sys.boundary = old_boundary
    return dW_of, undo, kT


def _apply_mc_barostat(sys, barostat, step_n, rng, energy=None):
    """apply_coupling!(sys, buffers, ::MonteCarloBarostat, sim, neighbors, step_n; rng) (coupling.jl:861-884).  `energy`: the potential-energy function (tests
    put the oracle's here to replay the same random numbers on the CPU)."""
    sys._refuse_constrained("MonteCarloBarostat coupling")
    sys._refuse_sites("MonteCarloBarostat coupling")
    if step_n % barostat.n_steps != 0:
        return False
    energy = energy or (lambda s: potential_energy(s, step_n))
    T = sys.dtype.type
    rand = lambda: T(rng.random(dtype=sys.dtype))                 # rand(rng, T)
    n_molecules = len(sys)                                        # sys.topology === nothing
    recompute = False
    for _ in range(barostat.n_iterations):
        E = energy(sys)
        dW_of, undo, kT = _mc_attempt(sys, barostat, E, rand, n_molecules)
        dW = dW_of(energy(sys))
        if dW <= 0 or float(rand()) < math.exp(-dW / kT):
            recompute = True
            barostat.n_accepted += 1
        else:
            undo()
        barostat.n_attempted += 1
    if barostat.n_attempted >= 10:                                # coupling.jl:871-881
        V_now = volume(sys.boundary)
        if barostat.n_accepted < 0.25 * barostat.n_attempted:
            barostat.volume_scale /= barostat.scale_increment
        elif barostat.n_accepted > 0.75 * barostat.n_attempted:
            barostat.volume_scale = min(barostat.volume_scale * barostat.scale_increment, V_now * barostat.max_volume_frac)
        barostat.n_attempted = 0
        barostat.n_accepted = 0
    return recompute


def wrap_coords(coords, boundary):
    """wrap_coords(v, boundary) (spatial.jl:573-602)"""
    c = np.asarray(coords)
    if isinstance(boundary, TriclinicBoundary):
        T = c.dtype.type
        bv = boundary.basis_vectors.astype(c.dtype); rs = (T(1) / np.array([bv[0, 0], bv[1, 1], bv[2, 2]], dtype=c.dtype)).astype(c.dtype)
        a, b, cc = boundary.basis_vectors
        cot_bc = T(abs((b[1] * cc[1] + b[2] * cc[2]) / (b[1] * cc[2] - b[2] * cc[1])))
        cxz, cyz, cot_ab = T(cc[0] / abs(cc[2])), T(cc[1] / abs(cc[2])), T(b[0] / b[1])
        v = c.reshape(-1, 3).copy()
        v -= bv[2] * np.floor(v[:, 2] * rs[2])[:, None]
        v -= bv[1] * np.floor((v[:, 1] - v[:, 2] * cot_bc) * rs[1])[:, None]
        dx, dy = v[:, 2] * cxz, v[:, 2] * cyz
        v -= bv[0] * np.floor((v[:, 0] - dx - (v[:, 1] - dy) * cot_ab) * rs[0])[:, None]
        return v.reshape(c.shape)
    L = boundary.side_lengths.astype(c.dtype)
    return c - np.floor(c / L) * L
