# BOHipAcq.jl -- LogEI and the acquisition functors on their own (include/bohip_acq.h, DESIGN.md 6k); included by BOHip.jl, inside
# its module.  Binds exactly the symbol of that header (checked mechanically in tests/test_logei_host.py).
c_acq_eval(acq, p, n, mu, var, value, dmu, dvar) = ccall((:bohip_acq_eval, libbohip), Cint, (Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), acq, p, n, mu, var, value, dmu, dvar)
const ACQ_LOGEI = Cint(6)           # BOHIP_ACQ_LOGEI
const LOGEI_SWITCH = -4.0           # csrc/acq_log.h: direct form above, Mills' ratio by its continued fraction below
const LOGEI_CF_DEPTH = 40

"""
    LogExpectedImprovement(; τ = -Inf)

An extension (the reference has no such type; no default uses it): the logarithm of the TEXTBOOK expected improvement,
log(Δ Φ(z) + σ φ(z)) = log σ + log h(z), h(z) = φ(z) + z Φ(z), in forms that stay finite and accurate for any z = (μ - τ) / σ.
Its arg-max is that of the textbook EI, and its gradient never vanishes where `ExpectedImprovement` underflows to 0.
`setparams!` follows `ExpectedImprovement`: τ ← max(maxy(model), τ).
"""
mutable struct LogExpectedImprovement <: AbstractAcquisition
    τ::Float64
end
LogExpectedImprovement(; τ = -Inf) = LogExpectedImprovement(τ)
setparams!(a::LogExpectedImprovement, model) = a.τ = max(maxy(model), a.τ)
acqid(::LogExpectedImprovement) = ACQ_LOGEI
acqparams(a::LogExpectedImprovement) = [a.τ, 0.0]

# (log h, Φ / h, φ / h) in the operations and order of csrc/acq_log.h
function logei_parts(z::Float64)
    if z > LOGEI_SWITCH
        ϕ = 0.3989422804014327 * exp(-0.5 * (z * z))
        Φ = 0.5 * erfc_(-z / 1.4142135623730951)
        h = ϕ + z * Φ
        return log(h), Φ / h, ϕ / h
    end
    t = -z; r = 0.0
    for k in LOGEI_CF_DEPTH:-1:2
        r = k / (t + r)
    end
    tr = t + r; c1 = 1.0 / tr; tc = t + c1
    -0.5 * (z * z) - 0.9189385332046728 + log(c1 / tc), tr, tc * tr
end
erfc_(x) = ccall(:erfc, Float64, (Float64,), x)     # libm's (no SpecialFunctions dependency)
function (a::LogExpectedImprovement)(μ, σ²)
    σ² == 0 && return μ > a.τ ? log(μ - a.τ) : -Inf
    σ = sqrt(σ²)
    log(σ) + logei_parts((μ - a.τ) / σ)[1]
end

"""
    acq_eval(a, μ, σ²; partials = true) -> (value, ∂/∂μ, ∂/∂σ²)

The functor `a` (ids 0-4 and 6) and its partials on the pairs (μ[i], σ²[i]), computed on the device by the functions the scoring
kernels inline.  No model is involved.
"""
function acq_eval(a::AbstractAcquisition, μ::AbstractVector, σ²::AbstractVector; partials::Bool = true)
    n = length(μ); length(σ²) == n || throw(DimensionMismatch("μ and σ² differ in length"))
    mu = Vector{Float64}(μ); var = Vector{Float64}(σ²)
    v = Vector{Float64}(undef, n); dm = Vector{Float64}(undef, n); dv = Vector{Float64}(undef, n)
    check(c_acq_eval(acqid(a), acqparams(a), n, mu, var, v, partials ? dm : C_NULL, partials ? dv : C_NULL))
    partials ? (v, dm, dv) : (v, nothing, nothing)
end
