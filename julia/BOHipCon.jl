# BOHipCon.jl -- constrained optimisation: feasibility-weighted acquisitions over several models, and the posterior's own Jacobians
# (include/bohip_con.h, DESIGN.md 6p); included by BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked
# mechanically in tests/test_con_host.py).
c_gp_predict_grad(h, Xs, R, mu, var, dmu, dvar) = ccall((:bohip_gp_predict_grad, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, Xs, R, mu, var, dmu, dvar)
c_con_values(h, acq, params, C, thr, senses, mu, var, R, value, logfeas, dmu, dvar, best) = ccall((:bohip_con_values, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, params, C, thr, senses, mu, var, R, value, logfeas, dmu, dvar, best)
c_gp_score_con(h, acq, params, C, cons, thr, senses, Xs, R, score, logfeas, grad, mu, var, best) = ccall((:bohip_gp_score_con, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Ptr{Cvoid}}, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, params, C, cons, thr, senses, Xs, R, score, logfeas, grad, mu, var, best)
const CON_CMAX = 16                 # BOHIP_CON_CMAX
const CON_FEASIBILITY = Cint(-1)    # BOHIP_CON_FEASIBILITY
const CON_ACQ = Dict(:EI => Cint(0), :PI => Cint(1), :LogEI => Cint(6), :Feasibility => CON_FEASIBILITY)

"""
    predict_grad(m, X) -> (mu, var, dmu, dvar)

An extension: the posterior at the columns of X together with its own Jacobians, `dmu` = ∇μ and `dvar` = ∇σ² (d x R, reported
unmasked: where var == 0 the clamp is the caller's).  What a score over several models is differentiated through.
"""
function predict_grad(m::AbstractBOHipModel, X::AbstractMatrix)
    Xc = _cols(m, X); R = size(Xc, 2); d = size(Xc, 1)
    μ = Vector{Float64}(undef, R); σ² = Vector{Float64}(undef, R)
    dμ = Matrix{Float64}(undef, d, R); dσ² = Matrix{Float64}(undef, d, R)
    check(c_gp_predict_grad(gp_handle(m), Xc, R, μ, σ², dμ, dσ²))
    μ, σ², dμ, dσ²
end

_con_acq(acq::Symbol) = haskey(CON_ACQ, acq) ? CON_ACQ[acq] :
    throw(ArgumentError("a constrained score takes :EI, :PI, :LogEI or :Feasibility: a signed score has no product form"))

"""
    con_values(m, acq, params, thresholds, senses, mu, var; want_grad = false)
        -> (value, logfeas, dmu, dvar, best value, 1-based best index)

The combine stage of `score_constrained` alone on the caller's moments: `mu`, `var` are R x (C + 1) (column 1 the objective, the
layout the library reads as (C + 1) x R row-major).  dmu and dvar are `nothing` without `want_grad`.  The model supplies the device
and the stream only.
"""
function con_values(m::AbstractBOHipModel, acq::Symbol, params, thresholds::AbstractVector, senses::AbstractVector,
                    mu::AbstractMatrix, var::AbstractMatrix; want_grad::Bool = false)
    C = length(thresholds)
    C == length(senses) || throw(DimensionMismatch("thresholds and senses differ in length"))
    size(mu) == size(var) && size(mu, 2) == C + 1 || throw(DimensionMismatch("mu and var must be R x (C + 1)"))
    μ = Matrix{Float64}(mu); σ² = Matrix{Float64}(var); R = size(μ, 1)
    p = vcat(Float64.(collect(params)), [0.0, 0.0]); t = Vector{Float64}(thresholds); s = Vector{Cint}(senses)
    vals = Vector{Float64}(undef, R); lf = Vector{Float64}(undef, R); best = Ref(Best(-Inf, -1))
    if want_grad
        dμ = Matrix{Float64}(undef, R, C + 1); dσ² = Matrix{Float64}(undef, R, C + 1)
        check(c_con_values(gp_handle(m), _con_acq(acq), p, C, t, s, μ, σ², R, vals, lf, dμ, dσ², best))
        return vals, lf, dμ, dσ², best[].val, Int(best[].idx) + 1
    end
    check(c_con_values(gp_handle(m), _con_acq(acq), p, C, t, s, μ, σ², R, vals, lf, C_NULL, C_NULL, best))
    vals, lf, nothing, nothing, best[].val, Int(best[].idx) + 1
end

"""
    score_constrained(objective, constraints, thresholds, senses, acq, params, X; want_grad = false)
        -> (scores, logfeas, grad, mu, var, best value, 1-based best column (0: nothing could win))

An extension (the reference's acquisition closes over one model): the acquisition `acq` of the objective weighted by the
probability that every constraint holds -- `:EI`, `:PI`: a exp(L); `:LogEI`: a + L; `:Feasibility`: L alone, L = Σ_c log Φ(s_c
(μ_c - t_c) / σ_c) -- over the columns of X in ONE library call.  `grad` (d x R) is `nothing` without `want_grad`; `mu`, `var` are
R x (C + 1).  The models live on one device and share the dimension.
"""
function score_constrained(objective::AbstractBOHipModel, constraints::AbstractVector, thresholds::AbstractVector,
                           senses::AbstractVector, acq::Symbol, params, X::AbstractMatrix; want_grad::Bool = false)
    C = length(constraints)
    C == length(thresholds) == length(senses) || throw(DimensionMismatch("constraints, thresholds and senses differ in length"))
    0 <= C <= CON_CMAX || throw(ArgumentError("0:$CON_CMAX constraints are supported"))
    Xc = _cols(objective, X); R = size(Xc, 2); d = size(Xc, 1)
    p = vcat(Float64.(collect(params)), [0.0, 0.0]); t = Vector{Float64}(thresholds); s = Vector{Cint}(senses)
    hs = Ptr{Cvoid}[gp_handle(c) for c in constraints]
    sc = Vector{Float64}(undef, R); lf = Vector{Float64}(undef, R)
    μ = Matrix{Float64}(undef, R, C + 1); σ² = Matrix{Float64}(undef, R, C + 1); best = Ref(Best(-Inf, -1))
    g = want_grad ? Matrix{Float64}(undef, d, R) : nothing
    GC.@preserve constraints check(c_gp_score_con(gp_handle(objective), _con_acq(acq), p, C, hs, t, s, Xc, R, sc, lf,
                                                  want_grad ? g : C_NULL, μ, σ², best))
    sc, lf, g, μ, σ², best[].val, Int(best[].idx) + 1
end
