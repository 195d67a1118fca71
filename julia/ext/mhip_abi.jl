# mhip_abi.jl — what both Julia front ends of libmollyhip.so share (include()d by ext/MollyHIPExt.jl and by MollyHIP/src/MollyHIP.jl): the C structs of
# include/mollyhip.h (same field order, LP64), the context table, error handling, and the pairwise_inters → mhip_interactions mapping.
# Needs `using Molly, Unitful` in the including module.
const libmollyhip = get(ENV, "MOLLYHIP_LIB", joinpath(get(ENV, "MOLLYHIP_ROOT", pwd()), "molly.jl_amd", "libmollyhip.so"))

# ---- C structs of include/mollyhip.h (same field order, LP64) -------------------------------------------------------
struct MhipInteractions
    lj_enabled::Int32; lj_cutoff_kind::Int32; lj_rc::Float64; lj_ra::Float64; lj_weight_special::Float64
    coul_kind::Int32; coul_cutoff_kind::Int32; coul_rc::Float64; coul_ra::Float64; coul_ke::Float64
    coul_weight_special::Float64; rf_dielectric::Float64; ewald_alpha::Float64; ewald_approx_erfc::Int32; reserved::Int32
end
struct MhipConfig
    precision::Int32; device_id::Int32; n_atoms::Int64
    box::NTuple{3, Float64}; origin::NTuple{3, Float64}; periodic::NTuple{3, Int32}
    rebuild_every::Int32; r_list::Float64; inter::MhipInteractions
end

# ---- context table ---------------------------------------------------------------------------------------------------
mutable struct HipContext
    ptr::Ptr{Cvoid}
    exceptions_generation::UInt64          # nf.cache_generation the engine's exception lists were built from
    bonded_sent::Bool
    boundary::Any                          # the sys.boundary the engine's box was made from (follow_boundary!)
    atoms::Any                             # the sys.atoms array the engine's parameters were read from (=== : a replaced array is pushed again)
    inters::Any                            # the sys.pairwise_inters tuple mhip_create fixed the kinds and cutoffs from (a replaced tuple: a new context)
    function HipContext(ptr, boundary=nothing)
        c = new(ptr, typemax(UInt64), false, boundary, nothing, nothing)
        finalizer(c) do x                   # GC-driven release; release!(sys) is the eager form
            x.ptr == C_NULL || ccall((:mhip_destroy, libmollyhip), Int32, (Ptr{Cvoid},), x.ptr)
            x.ptr = C_NULL
        end
        return c
    end
end
const CONTEXTS = IdDict{Any, HipContext}()      # System object → its engine context (the interactions that walk the neighbour list)
const CONTEXTS_NOLIST = IdDict{Any, HipContext}()   # System object → the context of its use_neighbors = false interactions (NoNeighborList, force.jl:1219-1224): every pair, no exceptions
const CONTEXTS_LOCK = ReentrantLock()

last_error(ptr) = unsafe_string(ccall((:mhip_last_error, libmollyhip), Cstring, (Ptr{Cvoid},), ptr))
check(c::HipContext, rc) = rc == 0 ? nothing : error("libmollyhip: ", last_error(c.ptr))     # ≙ error(...) of ext:733-739

# `sys.boundary = …` on a live system (scale_coords!, spatial.jl:1202; a barostat's rejected move, coupling.jl:930): the reference's entry points read
# sys.boundary at every call (ext/MollyCUDAExt.jl:845, 936), so every look-up of a context compares it with the boundary the engine holds and hands a new one
# over (mhip_set_box: grid, capacities and reciprocal box made again, lists dropped; the caller's mhip_set_state that follows brings the scaled coordinates).
function follow_boundary!(c::HipContext, b)
    c.boundary === b && return c
    if c.boundary !== nothing
        typeof(b).name === typeof(c.boundary).name || error("libmollyhip: a live System keeps its kind of boundary")
        if hasproperty(b, :basis_vectors)                                              # TriclinicBoundary (spatial.jl:151-161)
            bv = Float64[ustrip(b.basis_vectors[r][k]) for r in 1:3 for k in 1:3]
            box = Float64[bv[1], bv[5], bv[9]]
            check(c, ccall((:mhip_set_box, libmollyhip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c.ptr, box, bv))
        else                                                                           # CubicBoundary (spatial.jl:40)
            box = Float64[ustrip(x) for x in b.side_lengths]
            check(c, ccall((:mhip_set_box, libmollyhip), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), c.ptr, box, Ptr{Float64}(C_NULL)))
        end
    end
    c.boundary = b
    return c
end

function release!(sys; table=nothing)
    lock(CONTEXTS_LOCK) do
        for t in (table === nothing ? (CONTEXTS, CONTEXTS_NOLIST) : (table,))
            c = pop!(t, sys, nothing)
            c === nothing || finalize(c)
        end
    end
    return nothing
end

# ---- pairwise_inters → mhip_interactions ----------------------------------------------------------------------------
cutoff_kind(::NoCutoff) = Int32(0); cutoff_kind(::DistanceCutoff) = Int32(1); cutoff_kind(::ShiftedPotentialCutoff) = Int32(2)
cutoff_kind(::ShiftedForceCutoff) = Int32(3); cutoff_kind(::CubicSplineCutoff) = Int32(4); cutoff_kind(::PolynomialCutoff) = Int32(5)
cutoff_rc(::NoCutoff) = 0.0;                 cutoff_rc(c) = Float64(ustrip(c.dist_cutoff))           # cutoffs.jl:72-253
cutoff_ra(c::Union{CubicSplineCutoff, PolynomialCutoff}) = Float64(ustrip(c.dist_activation)); cutoff_ra(c) = 0.0

function interactions(inters::Tuple)
    lj = (Int32(0), Int32(0), 0.0, 0.0, 1.0)
    coul = (Int32(0), Int32(0), 0.0, 0.0, 138.93545764, 1.0, 1.0, 0.0, Int32(1))     # kind, cutoff, rc, ra, ke, w14, ε_rf, α, approx
    n_lj = n_coul = 0
    for inter in inters
        if inter isa LennardJones                                                    # lennard_jones.jl:25-47
            n_lj += 1
            lj = (Int32(1), cutoff_kind(inter.cutoff), cutoff_rc(inter.cutoff), cutoff_ra(inter.cutoff), Float64(inter.weight_special))
        elseif inter isa Coulomb                                                     # coulomb.jl:32-69
            n_coul += 1
            coul = (Int32(1), cutoff_kind(inter.cutoff), cutoff_rc(inter.cutoff), cutoff_ra(inter.cutoff),
                    Float64(ustrip(inter.coulomb_const)), Float64(inter.weight_special), 1.0, 0.0, Int32(1))
        elseif inter isa CoulombReactionField                                        # coulomb.jl:698-746
            n_coul += 1
            coul = (Int32(2), Int32(0), Float64(ustrip(inter.dist_cutoff)), 0.0, Float64(ustrip(inter.coulomb_const)),
                    Float64(inter.weight_special), Float64(inter.solvent_dielectric), 0.0, Int32(1))
        elseif inter isa CoulombEwald                                                # coulomb.jl:1320-1382
            n_coul += 1
            coul = (Int32(3), Int32(0), Float64(ustrip(inter.dist_cutoff)), 0.0, Float64(ustrip(inter.coulomb_const)),
                    Float64(inter.weight_special), 1.0, Float64(ustrip(inter.α)), Int32(inter.approximate_erfc))
        else
            error("MollyHIPExt: pairwise interaction $(typeof(inter)) is outside the engine's scope (LennardJones, Coulomb, CoulombReactionField, CoulombEwald)")
        end
    end
    (n_lj <= 1 && n_coul <= 1) || error("MollyHIPExt: at most one LennardJones and one Coulomb-type interaction")
    return MhipInteractions(lj[1], lj[2], lj[3], lj[4], lj[5], coul[1], coul[2], coul[3], coul[4], coul[5], coul[6], coul[7], coul[8], coul[9], 0)
end

# one timed candidate of mhip_optimize_launch_config (mhip_launch_trial)
struct MhipLaunchTrial
    block_atoms::Int32
    j_split::Int32
    us_per_pass::Float32
end

# ---- raw wrappers (no reference generic is overridden) ----------------------------------------------------------------
# mhip_constraint_virial: the constraint contribution to the virial at the coordinates and velocities the context holds, by the trial step of
# merge_initial_constraint_virial! (simulators.jl:459-495; per-cluster accumulation shake.jl:234-392), ADDED to virial9 (3×3, row-major); parts18 is
# written with the RATTLE part then the SHAKE part.  f: the total forces in the context's precision (3 × n_atoms, the memory order of
# Array(reinterpret(T, fs))), virtual-site rows already distributed.  Returns the cluster solves of this call that stopped at max_iters.  For a pressure
# logger or a Julia-side barostat of a constrained System, next to the force virial of mhip_forces / mhip_specific_virial / mhip_general_virial.
function constraint_virial!(virial9::Vector{Float64}, parts18::Vector{Float64}, c::HipContext, f::Array{T}; dt::Float64=0.0005) where {T<:Union{Float32, Float64}}
    (length(virial9) == 9 && length(parts18) == 18) || error("libmollyhip: constraint_virial! takes 9 and 18 doubles")
    n_not_converged = Ref{Int64}(0)
    check(c, ccall((:mhip_constraint_virial, libmollyhip), Int32, (Ptr{Cvoid}, Ptr{T}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
                   c.ptr, f, 0, dt, virial9, parts18, n_not_converged))
    return n_not_converged[]
end

# mhip_minimize: the steepest-descent loop of simulators.jl:183-271 on the coordinates the context holds, with its decisions taken on the device.
# constraint_bond_k > 0 puts a harmonic bond k/2·(r − d)² on every constrained pair for the duration (constraints_to_bonds, constraints.jl:619-636), 0 ignores
# the constraints.  log4 (4 × max_steps): per step taken E_trial, max_force, accepted, the hn it moved by.  Returns out8 = (initial E, final E, last max_force,
# final hn, steps taken, accepted, rejected, converged).
function minimize!(log4::Matrix{Float64}, c::HipContext; first_step::Integer=0, max_steps::Integer=1000, step_size::Float64=0.01, tol::Float64=1000.0,
                   constraint_bond_k::Float64=500_000.0)
    size(log4) == (4, max_steps) || error("libmollyhip: minimize! takes a 4 × max_steps log")
    out8 = zeros(Float64, 8)
    check(c, ccall((:mhip_minimize, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
                   c.ptr, first_step, max_steps, step_size, tol, constraint_bond_k, log4, out8))
    return out8
end

# mhip_splitting_run: simulate!(sys, ::LangevinSplitting, n) (simulators.jl:1255-1381) on the state the context holds.  splitting: 1 to 16 characters out of A, B, O
# with at most one force computation per step (the engine's limits); friction is the reference's mass-per-time quantity; kT = temperature·k.  The k-th O
# (0-based) of step first_step + s draws from philox_ctr1 + (s − 1)·n_O + k, so a continued run passes philox_ctr1 + steps_done·count('O', splitting).
function splitting_run!(c::HipContext, splitting::AbstractString; first_step::Integer=0, n_steps::Integer, dt::Float64, kT::Float64, friction::Float64,
                        remove_cm_every::Integer=1, philox_key::UInt64=UInt64(0), philox_ctr1::UInt64=UInt64(0))
    check(c, ccall((:mhip_splitting_run, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Cstring, Int32, UInt64, UInt64),
                   c.ptr, first_step, n_steps, dt, kT, friction, String(splitting), remove_cm_every, philox_key, philox_ctr1))
    return c
end

# mhip_overdamped_run: simulate!(sys, ::OverdampedLangevin, n) (simulators.jl:1426-1489), Euler–Maruyama; friction is an inverse time.  Step first_step + s draws
# from (philox_key, philox_ctr1 + s − 1) — one key and a counter where the reference draws a fresh pair per step — and remove_CM_motion! is applied to the
# (otherwise untouched) velocities once per call.
function overdamped_run!(c::HipContext; first_step::Integer=0, n_steps::Integer, dt::Float64, kT::Float64, friction::Float64, remove_cm_every::Integer=1,
                         philox_key::UInt64=UInt64(0), philox_ctr1::UInt64=UInt64(0))
    check(c, ccall((:mhip_overdamped_run, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int64, Float64, Float64, Float64, Int32, UInt64, UInt64),
                   c.ptr, first_step, n_steps, dt, kT, friction, remove_cm_every, philox_key, philox_ctr1))
    return c
end

# ---- the recorder: what apply_loggers! (loggers.jl:44-56) reads of a step, taken inside mhip_vv_run / mhip_langevin_run and kept on the device --------------
# Channels (0-based, as in mollyhip.h): 0 kinetic energy, 1 potential energy (pairwise, specific, general), 2 coordinates, 3 velocities.  The simulate! methods
# of MollyHIPExt.jl still cut their runs at the logger intervals (run_chunks!): a caller who drives a HipContext directly records with these.
# mhip_set_record: every / capacity per channel (every = 0: off); all off gives the buffers back; always empties the history.
function set_record!(c::HipContext, every::Vector{Int32}, capacity::Vector{Int64})
    (length(every) == 4 && length(capacity) == 4) || error("libmollyhip: set_record! takes four intervals and four capacities")
    check(c, ccall((:mhip_set_record, libmollyhip), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ref{Int64}), c.ptr, every, capacity))
    return c
end

# mhip_record_now: the state held, under step number step_n, for the channels of the mask (bit c = channel c) — the loggers before the first step
# (simulators.jl:571) and between the calls of a run driven step by step
function record_now!(c::HipContext, step_n::Integer, channel_mask::Integer)
    check(c, ccall((:mhip_record_now, libmollyhip), Int32, (Ptr{Cvoid}, Int64, Int32), c.ptr, step_n, channel_mask))
    return c
end

# mhip_record_info: per channel (every, capacity, records held, step of the last record or -1), a 4 × 4 matrix with one column per channel
function record_info(c::HipContext)
    out16 = zeros(Int64, 4, 4)
    check(c, ccall((:mhip_record_info, libmollyhip), Int32, (Ptr{Cvoid}, Ref{Int64}), c.ptr, out16))
    return out16
end

# mhip_record_read: records first … first + n − 1 (0-based) of a channel into host memory (≙ values(logger), loggers.jl:96-102): Float64 for channels 0 and 1
# (1 and 3 values per record), the context's precision for the frames (3 × n_atoms per record).  Returns the records' step numbers.
function record_read!(values::Array{T}, c::HipContext, channel::Integer, first::Integer, n::Integer) where {T<:Union{Float32, Float64}}
    steps = zeros(Int64, n)
    check(c, ccall((:mhip_record_read, libmollyhip), Int32, (Ptr{Cvoid}, Int32, Int64, Int64, Ref{Int64}, Ptr{Cvoid}, Int32), c.ptr, channel, first, n, steps, values, 0))
    return steps
end

# mhip_record_clear: empties the history, keeps intervals and buffers
function record_clear!(c::HipContext)
    check(c, ccall((:mhip_record_clear, libmollyhip), Int32, (Ptr{Cvoid},), c.ptr))
    return c
end
