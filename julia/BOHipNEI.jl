# BOHipNEI.jl -- noisy expected improvement (include/bohip_nei.h, DESIGN.md 6v); included by BOHip.jl, inside its module.  Binds exactly
# the symbols of that header (checked mechanically in tests/test_nei_host.py).  Like the rest of the binding it has never been executed:
# there is no Julia toolchain where the library is built; the functions restate the Python host layer
# (bayesianoptimization.jl_amd/model.py, acquisition.py) statement for statement.
c_gp_nei_prepare(h, jrel, S, seed) = ccall((:bohip_gp_nei_prepare, libbohip), Cint, (Ptr{Cvoid}, Float64, Int64, UInt64), h, jrel, S, seed)
c_gp_nei_fantasies(h, jrel, S, seed, F, tau) = ccall((:bohip_gp_nei_fantasies, libbohip), Cint, (Ptr{Cvoid}, Float64, Int64, UInt64, Ptr{Float64}, Ptr{Float64}), h, jrel, S, seed, F, tau)
c_gp_score_nei(h, acq, prm, Xs, R, S, seed, jrel, sc, mu, var, best) = ccall((:bohip_gp_score_nei, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, prm, Xs, R, S, seed, jrel, sc, mu, var, best)
c_nei_values(h, acq, R, S, mus, var, tau, sc, mm, best) = ccall((:bohip_nei_values, libbohip), Cint, (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, R, S, mus, var, tau, sc, mm, best)
c_gp_nei_info(h, what, v) = ccall((:bohip_gp_nei_info, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}), h, what, v)
c_gp_nei_release(h) = ccall((:bohip_gp_nei_release, libbohip), Cint, (Ptr{Cvoid},), h)

const NEI_SMAX = 1024       # BOHIP_NEI_SMAX
const NEI_ACQ = Dict(:ei => Cint(0), :pi => Cint(1), :logei => Cint(6))
const NEI_INFO = (refits = Cint(0), appends = Cint(1), rebuilds = Cint(2), jitter_steps = Cint(3), bytes = Cint(4), delta = Cint(5))

"""
    nei(m, X; S = 32, seed = 0, acq = :ei, jitter_rel = 1e-8) -> (score, mu, var, best value, 1-based best column, tau)

Noisy expected improvement at the columns of `X` (bohip_gp_score_nei; Letham, Karrer, Ottoni & Bakshy 2019, eq. 6): `acq` (:ei, :pi or
:logei) averaged over `S` posterior draws of the noise-free function values at the observed sites, each with its own incumbent.
`S = 0`: the plug-in form.  `mu` is the mean over the draws of m_s, `var` the shared noise-free variance, `tau` the incumbents.  On a
device list the first replica runs it.  The model is not changed.
"""
function nei(m::AbstractBOHipModel, X::AbstractMatrix; S::Integer = 32, seed::Integer = 0, acq::Symbol = :ei, jitter_rel::Real = 1e-8)
    haskey(NEI_ACQ, acq) || throw(ArgumentError("acq must be :ei, :pi or :logei"))
    Xc = _cols(m, X); R = size(Xc, 2)
    sc = Vector{Float64}(undef, R); mu = similar(sc); var = similar(sc); tau = Vector{Float64}(undef, max(S, 1))
    best = Ref(Best(-Inf, -1))
    check(c_gp_nei_fantasies(gp_handle(m), Float64(jitter_rel), S, UInt64(seed), C_NULL, tau))
    check(c_gp_score_nei(gp_handle(m), NEI_ACQ[acq], C_NULL, Xc, R, S, UInt64(seed), Float64(jitter_rel), sc, mu, var, best))
    sc, mu, var, best[].val, Int(best[].idx) + 1, tau
end

"(F, tau): the fantasised noise-free function values at the observed sites, max(S, 1) x n with row s = f_s, and their maxima."
function nei_fantasies(m::AbstractBOHipModel; S::Integer = 32, seed::Integer = 0, jitter_rel::Real = 1e-8)
    S1 = max(S, 1); n = length(m.y)
    Ft = Matrix{Float64}(undef, n, S1); tau = Vector{Float64}(undef, S1)      # (the library writes row-major S1 x n)
    check(c_gp_nei_fantasies(gp_handle(m), Float64(jitter_rel), S, UInt64(seed), Ft, tau))
    permutedims(Ft), tau
end

"Brings the model, its noise-free companion and the fantasies up to date (optional: `nei` does the same lazily)."
function nei_prepare!(m::AbstractBOHipModel; S::Integer = 32, seed::Integer = 0, jitter_rel::Real = 1e-8)
    check(c_gp_nei_prepare(gp_handle(m), Float64(jitter_rel), S, UInt64(seed)))
    m
end

"The averaging stage on its own: mu_s (R x S), var (R), tau_s (S) -> (scores, mean over s of mu_s, best value, 1-based best row)."
function nei_values(m::AbstractBOHipModel, acq::Symbol, mu_s::AbstractMatrix, var::AbstractVector, tau_s::AbstractVector)
    haskey(NEI_ACQ, acq) || throw(ArgumentError("acq must be :ei, :pi or :logei"))
    R, S = size(mu_s)
    length(var) == R && length(tau_s) == S || throw(DimensionMismatch("mu_s (R x S), var (R) and tau_s (S) disagree"))
    Mt = Matrix{Float64}(permutedims(mu_s))                                    # (the library reads row-major R x S)
    sc = Vector{Float64}(undef, R); mm = similar(sc)
    best = Ref(Best(-Inf, -1))
    check(c_nei_values(gp_handle(m), NEI_ACQ[acq], R, S, Mt, Vector{Float64}(var), Vector{Float64}(tau_s), sc, mm, best))
    sc, mm, best[].val, Int(best[].idx) + 1
end

"A quantity of NEI_INFO (:refits, :appends, :rebuilds, :jitter_steps, :bytes, :delta) of the model's noise-free companion."
function nei_info(m::AbstractBOHipModel, what::Symbol)
    v = Ref{Float64}(0.0)
    check(c_gp_nei_info(gp_handle(m), getfield(NEI_INFO, what), v))
    what === :delta ? v[] : Int(v[])
end

"Frees the companion and the fantasies; the next call builds them again."
function nei_release!(m::AbstractBOHipModel)
    check(c_gp_nei_release(gp_handle(m)))
    m
end

"""
    NoisyExpectedImprovement(S = 32, seed = 0, log = false)

EI (with `log`: the logarithm of the averaged EI) averaged over `S` posterior draws of the noise-free function values at the observed
sites.  An extension: the reference has no such type and no default uses it.  No parameter follows the model and there is no gradient
in x: `acquire_max` takes the device's arg-max over `maxeval` Latin-hypercube candidates per restart.
"""
struct NoisyExpectedImprovement <: AbstractAcquisition
    S::Int
    seed::Int
    log::Bool
    function NoisyExpectedImprovement(S::Integer = 32, seed::Integer = 0, log::Bool = false)
        0 <= S <= NEI_SMAX || throw(ArgumentError("S must be in 0:$NEI_SMAX"))
        new(S, seed, log)
    end
end
setparams!(::NoisyExpectedImprovement, model) = nothing
function defaultoptions(::Type{<:AbstractBOHipModel}, ::Type{NoisyExpectedImprovement})
    (method = :LD_LBFGS, restarts = 1, maxeval = 1024)
end
function acquire_max_device(a::NoisyExpectedImprovement, m::AbstractBOHipModel, lowerbounds, upperbounds, options)
    _check_options(options)
    lb = Float64.(lowerbounds); ub = Float64.(upperbounds)
    maxf = -Inf; maxx = lb
    isempty(m.y) && return maxf, maxx
    for _ in 1:options.restarts
        cand = BO.latin_hypercube_sampling(lb, ub, max(options.maxeval, 1))
        _, _, _, f, j, _ = nei(m, cand; S = a.S, seed = a.seed, acq = a.log ? :logei : :ei)
        if j >= 1 && f > maxf                                     # src/acquisition.jl:62 strict '>'
            maxf = f; maxx = cand[:, j]
        end
    end
    maxf, maxx
end
