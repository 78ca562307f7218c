# BOHipMO.jl -- two-objective optimisation: the observed Pareto front and the exact expected hypervolume improvement over it
# (include/bohip_mo.h, DESIGN.md 6q); included by BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked
# mechanically in tests/test_mo_host.py).  Both objectives are maximised.
c_mo_front(Y, n, ref, front, cap, n_front, hv) = ccall((:bohip_mo_front, libbohip), Cint, (Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}), Y, n, ref, front, cap, n_front, hv)
c_mo_ehvi_values(h, front, n_front, ref, mu, var, R, value, dmu, dvar, best) = ccall((:bohip_mo_ehvi_values, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, front, n_front, ref, mu, var, R, value, dmu, dvar, best)
c_gp_score_mo(h0, h1, front, n_front, ref, Xs, R, score, grad, mu, var, best) = ccall((:bohip_gp_score_mo, libbohip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h0, h1, front, n_front, ref, Xs, R, score, grad, mu, var, best)
const MO_FRONT_MAX = 1024           # BOHIP_MO_FRONT_MAX
const MO_GROUP = 16                 # BOHIP_MO_GROUP

_mo_ref(ref) = length(ref) == 2 ? Vector{Float64}(collect(ref)) : throw(DimensionMismatch("the reference point has two coordinates"))

"""
    mo_front(Y, ref) -> (front, hv)

An extension (the reference optimises one objective).  `Y` is n x 2 (column m objective m, the layout the library reads as 2 x n
row-major).  `front` (n_front x 2) holds the observations that strictly dominate `ref` and are not weakly dominated by another,
ascending in the first objective; `hv` is the hypervolume it dominates above `ref`.  Host code: no device is needed.
"""
function mo_front(Y::AbstractMatrix, ref)
    size(Y, 2) == 2 || throw(DimensionMismatch("Y must be n x 2"))
    Yc = Matrix{Float64}(Y); n = size(Yc, 1); r = _mo_ref(ref)
    nf = Ref{Int64}(0); hv = Ref{Float64}(0.0)
    out = Matrix{Float64}(undef, max(n, 1), 2)
    check(c_mo_front(Yc, n, r, out, size(out, 1), nf, hv))
    out[1:nf[], :], hv[]
end

"""
    ehvi_values(m, front, ref, mu, var; want_grad = false) -> (value, dmu, dvar, best value, 1-based best index)

The EHVI stage alone on the caller's moments: `front` as `mo_front` returns it (n_front x 2), `mu`, `var` R x 2.  dmu and dvar
(R x 2) are `nothing` without `want_grad`.  The model supplies the device and the stream only.
"""
function ehvi_values(m::AbstractBOHipModel, front::AbstractMatrix, ref, mu::AbstractMatrix, var::AbstractMatrix; want_grad::Bool = false)
    size(front, 2) == 2 || throw(DimensionMismatch("front must be n_front x 2"))
    size(mu) == size(var) && size(mu, 2) == 2 || throw(DimensionMismatch("mu and var must be R x 2"))
    F = Matrix{Float64}(front); μ = Matrix{Float64}(mu); σ² = Matrix{Float64}(var); R = size(μ, 1); r = _mo_ref(ref)
    vals = Vector{Float64}(undef, R); best = Ref(Best(-Inf, -1))
    if want_grad
        dμ = Matrix{Float64}(undef, R, 2); dσ² = Matrix{Float64}(undef, R, 2)
        check(c_mo_ehvi_values(gp_handle(m), F, size(F, 1), r, μ, σ², R, vals, dμ, dσ², best))
        return vals, dμ, dσ², best[].val, Int(best[].idx) + 1
    end
    check(c_mo_ehvi_values(gp_handle(m), F, size(F, 1), r, μ, σ², R, vals, C_NULL, C_NULL, best))
    vals, nothing, nothing, best[].val, Int(best[].idx) + 1
end

"""
    score_mo(obj0, obj1, front, ref, X; want_grad = false)
        -> (scores, grad, mu, var, best value, 1-based best column (0: nothing could win))

An extension: the exact expected hypervolume improvement of the two models' posteriors over `front` above `ref`, over the columns
of X in ONE library call.  `grad` (d x R) is `nothing` without `want_grad`; `mu`, `var` are R x 2.  The models live on one device
and share the dimension.
"""
function score_mo(obj0::AbstractBOHipModel, obj1::AbstractBOHipModel, front::AbstractMatrix, ref, X::AbstractMatrix; want_grad::Bool = false)
    size(front, 2) == 2 || throw(DimensionMismatch("front must be n_front x 2"))
    F = Matrix{Float64}(front); r = _mo_ref(ref)
    Xc = _cols(obj0, X); R = size(Xc, 2); d = size(Xc, 1)
    sc = Vector{Float64}(undef, R); μ = Matrix{Float64}(undef, R, 2); σ² = Matrix{Float64}(undef, R, 2); best = Ref(Best(-Inf, -1))
    g = want_grad ? Matrix{Float64}(undef, d, R) : nothing
    GC.@preserve obj1 check(c_gp_score_mo(gp_handle(obj0), gp_handle(obj1), F, size(F, 1), r, Xc, R, sc, want_grad ? g : C_NULL, μ, σ², best))
    sc, g, μ, σ², best[].val, Int(best[].idx) + 1
end
