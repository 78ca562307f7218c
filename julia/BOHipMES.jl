# BOHipMES.jl -- max-value entropy search over a candidate set, on the device (include/bohip_mes.h, DESIGN.md 6o); included by
# BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked mechanically in tests/test_mes_host.py).
c_gp_mes(h, Xs, R, K, mode, seed, floor, jitter_rel, max_tries, mes, maxvals, quantiles, mu, var, best, jitter_used, tries_used) = ccall((:bohip_gp_mes, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Cint, UInt64, Float64, Float64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}, Ptr{Float64}, Ptr{Cint}), h, Xs, R, K, mode, seed, floor, jitter_rel, max_tries, mes, maxvals, quantiles, mu, var, best, jitter_used, tries_used)
c_mes_values(h, mu, var, R, maxvals, K, mes, dmu, dvar, best) = ccall((:bohip_mes_values, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, mu, var, R, maxvals, K, mes, dmu, dvar, best)
c_mes_gumbel(h, mu, var, R, K, seed, floor, quantiles, maxvals) = ccall((:bohip_mes_gumbel, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Float64, Ptr{Float64}, Ptr{Float64}), h, mu, var, R, K, seed, floor, quantiles, maxvals)
const MES_KMAX = 1024               # BOHIP_MES_KMAX
const MES_RMAX = 524288             # BOHIP_MES_RMAX
const MES_MODES = Dict(:gumbel => Cint(0), :joint => Cint(1))

"""
    mes(m, X; samples = 16, mode = :gumbel, seed = 0, floor = -Inf, jitter_rel = 1e-12, max_tries = 40)
        -> (values, maxvals, quantiles, mu, var, best value, 1-based best column (0: nothing could win))

An extension (the reference has no such acquisition): max-value entropy search (Wang & Jegelka 2017) over the candidate set X,
MES_j = mean_k u(mu_j, s2_j, m_k) over `samples` draws m_k of the maximum of the posterior over the candidates.  `:gumbel` fits a
Gumbel law to three quantiles of the maximum of independent candidates; `:joint` takes the row maxima of the joint draws of
`sample_joint` for the same arguments (R within one chunk; the quantiles are NaN).  Everything stays on the device.  The model is
not changed.  On a device list the first replica runs it.
"""
function mes(m::AbstractBOHipModel, X::AbstractMatrix; samples::Integer = 16, mode::Symbol = :gumbel, seed::Integer = 0,
             floor::Real = -Inf, jitter_rel::Real = 1e-12, max_tries::Integer = 40)
    haskey(MES_MODES, mode) || throw(ArgumentError("mode must be :gumbel or :joint"))
    Xc = _cols(m, X); R = size(Xc, 2)
    vals = Vector{Float64}(undef, R); μ = Vector{Float64}(undef, R); σ² = Vector{Float64}(undef, R)
    mv = Vector{Float64}(undef, max(samples, 1)); q = Vector{Float64}(undef, 3)
    best = Ref(Best(-Inf, -1)); jit = Ref(0.0); tries = Ref(Cint(0))
    check(c_gp_mes(gp_handle(m), Xc, R, samples, MES_MODES[mode], UInt64(seed), Float64(floor), Float64(jitter_rel), Cint(max_tries),
                   vals, mv, q, μ, σ², best, jit, tries))
    vals, mv, q, μ, σ², best[].val, Int(best[].idx) + 1
end
"""
    mes_values(m, mu, var, maxvals; want_grad = false) -> (values, dmu, dvar, best value, 1-based best index)

The functor of `mes` alone on the caller's (mu, var, maxvals); dmu and dvar are `nothing` without `want_grad`.  The model supplies
the device and the stream only.
"""
function mes_values(m::AbstractBOHipModel, mu::AbstractVector, var::AbstractVector, maxvals::AbstractVector; want_grad::Bool = false)
    μ = Vector{Float64}(mu); σ² = Vector{Float64}(var); mv = Vector{Float64}(maxvals); R = length(μ)
    R == length(σ²) || throw(DimensionMismatch("mu and var differ in length"))
    vals = Vector{Float64}(undef, R); best = Ref(Best(-Inf, -1))
    if want_grad
        dμ = Vector{Float64}(undef, R); dσ² = Vector{Float64}(undef, R)
        check(c_mes_values(gp_handle(m), μ, σ², R, mv, length(mv), vals, dμ, dσ², best))
        return vals, dμ, dσ², best[].val, Int(best[].idx) + 1
    end
    check(c_mes_values(gp_handle(m), μ, σ², R, mv, length(mv), vals, C_NULL, C_NULL, best))
    vals, nothing, nothing, best[].val, Int(best[].idx) + 1
end
"""
    mes_gumbel(m, mu, var; samples = 16, seed = 0, floor = -Inf) -> (quantiles, maxvals)

The max-value sampler of mode `:gumbel` alone on the caller's (mu, var).
"""
function mes_gumbel(m::AbstractBOHipModel, mu::AbstractVector, var::AbstractVector; samples::Integer = 16, seed::Integer = 0,
                    floor::Real = -Inf)
    μ = Vector{Float64}(mu); σ² = Vector{Float64}(var)
    length(μ) == length(σ²) || throw(DimensionMismatch("mu and var differ in length"))
    q = Vector{Float64}(undef, 3); mv = Vector{Float64}(undef, max(samples, 1))
    check(c_mes_gumbel(gp_handle(m), μ, σ², length(μ), samples, UInt64(seed), Float64(floor), q, mv))
    q, mv
end

"""
    MaxValueEntropySearch(samples = 16, mode = :gumbel)

Max-value entropy search as an acquisition: a candidate-set acquisition without a gradient in x.  `acquire_max` takes `maxeval`
Latin-hypercube candidates per restart, one `mes` call each with a fresh seed, and keeps the first maximum over the restarts
(strict `>`); `method` is accepted and not used.
"""
struct MaxValueEntropySearch <: AbstractAcquisition
    samples::Int
    mode::Symbol
    function MaxValueEntropySearch(samples::Integer = 16, mode::Symbol = :gumbel)
        1 <= samples <= MES_KMAX || throw(ArgumentError("samples must be in 1:$MES_KMAX"))
        haskey(MES_MODES, mode) || throw(ArgumentError("mode must be :gumbel or :joint"))
        new(samples, mode)
    end
end
setparams!(::MaxValueEntropySearch, model) = nothing
function defaultoptions(::Type{<:AbstractBOHipModel}, ::Type{MaxValueEntropySearch})
    (method = :LD_LBFGS, restarts = 1, maxeval = 1024)
end
function acquire_max_device(a::MaxValueEntropySearch, m::AbstractBOHipModel, lowerbounds, upperbounds, options)
    _check_options(options)
    lb = Float64.(lowerbounds); ub = Float64.(upperbounds)
    maxf = -Inf; maxx = lb
    isempty(m.y) && return maxf, maxx
    for _ in 1:options.restarts
        cand = BO.latin_hypercube_sampling(lb, ub, max(options.maxeval, 1))
        _, _, _, _, _, f, j = mes(m, cand; samples = a.samples, mode = a.mode, seed = rand(UInt64) >> 1)
        if j >= 1 && f > maxf                                     # src/acquisition.jl:62 strict '>'
            maxf = f; maxx = cand[:, j]
        end
    end
    maxf, maxx
end
