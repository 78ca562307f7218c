# BOHipMOM.jl -- two to four objectives: the observed Pareto front, its decomposition into boxes and the exact expected
# hypervolume improvement as a sum over them (include/bohip_mom.h, DESIGN.md 6w); included by BOHip.jl, inside its module.  Binds
# exactly the symbols of that header (checked mechanically in tests/test_mom_host.py).  Every objective is maximised.
c_mom_front(Y, M, n, ref, front, cap, n_front, hv) = ccall((:bohip_mom_front, libbohip), Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}), Y, M, n, ref, front, cap, n_front, hv)
c_mom_boxes(front, M, n_front, ref, levels, n_levels, boxes, cap, n_boxes) = ccall((:bohip_mom_boxes, libbohip), Cint, (Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Int64}), front, M, n_front, ref, levels, n_levels, boxes, cap, n_boxes)
c_mom_ehvi_values(h, M, front, n_front, ref, mu, var, R, value, dmu, dvar, best) = ccall((:bohip_mom_ehvi_values, libbohip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, M, front, n_front, ref, mu, var, R, value, dmu, dvar, best)
c_gp_score_mom(objs, M, front, n_front, ref, Xs, R, score, grad, mu, var, best) = ccall((:bohip_gp_score_mom, libbohip), Cint, (Ptr{Ptr{Cvoid}}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), objs, M, front, n_front, ref, Xs, R, score, grad, mu, var, best)
const MOM_OBJ_MAX = 4               # BOHIP_MOM_OBJ_MAX
const MOM_FRONT_MAX = 256           # BOHIP_MOM_FRONT_MAX
const MOM_BOX_MAX = 65536           # BOHIP_MOM_BOX_MAX
const MOM_LANES = 64                # BOHIP_MOM_LANES

_mom_M(A, what) = 2 <= size(A, 2) <= MOM_OBJ_MAX ? size(A, 2) : throw(DimensionMismatch("$what has one column per objective, 2 to $MOM_OBJ_MAX"))
_mom_ref(ref, M) = length(ref) == M ? Vector{Float64}(collect(ref)) : throw(DimensionMismatch("the reference point has one coordinate per objective"))

"""
    mom_front(Y, ref) -> (front, hv)

An extension (the reference optimises one objective).  `Y` is n x M (column m objective m, the layout the library reads as M x n
row-major), M = 2 to 4.  `front` (n_front x M) holds the observations strictly above `ref` in every coordinate that no other
observation weakly dominates, in lexicographic ascending order; `hv` is the hypervolume it dominates above `ref`.  Host code: no
device is needed.
"""
function mom_front(Y::AbstractMatrix, ref)
    M = _mom_M(Y, "Y")
    Yc = Matrix{Float64}(Y); n = size(Yc, 1); r = _mom_ref(ref, M)
    nf = Ref{Int64}(0); hv = Ref{Float64}(0.0)
    out = Matrix{Float64}(undef, max(n, 1), M)
    check(c_mom_front(Yc, M, n, r, out, size(out, 1), nf, hv))
    out[1:nf[], :], hv[]
end

"""
    mom_boxes(front, ref) -> (levels, boxes)

The decomposition of the region above `ref` that no point of `front` (n_front x M) dominates: `levels[m]` holds ref[m], the
front's distinct values in objective m ascending, and Inf; `boxes` is n_boxes x 2M Int32, column m the lower and column M + m the
upper 0-based level index of every box in objective m.  Host code: no device is needed.
"""
function mom_boxes(front::AbstractMatrix, ref)
    M = _mom_M(front, "front")
    F = Matrix{Float64}(front); n = size(F, 1); r = _mom_ref(ref, M)
    L = Matrix{Float64}(undef, n + 2, M); nl = Vector{Int64}(undef, M); nb = Ref{Int64}(0)
    check(c_mom_boxes(F, M, n, r, L, nl, C_NULL, 0, nb))
    B = Matrix{Int32}(undef, nb[], 2M)
    check(c_mom_boxes(F, M, n, r, C_NULL, C_NULL, B, nb[], C_NULL))
    map(m -> L[1:nl[m], m], 1:M), B
end

"""
    ehvi_values_many(m, front, ref, mu, var; want_grad = false) -> (value, dmu, dvar, best value, 1-based best index)

The EHVI stage alone on the caller's moments: `front` n_front x M, `mu`, `var` R x M.  dmu and dvar (R x M) are `nothing` without
`want_grad`.  The model supplies the device and the stream only.
"""
function ehvi_values_many(m::AbstractBOHipModel, front::AbstractMatrix, ref, mu::AbstractMatrix, var::AbstractMatrix; want_grad::Bool = false)
    M = _mom_M(mu, "mu")
    size(mu) == size(var) || throw(DimensionMismatch("mu and var must both be R x M"))
    size(front, 2) == M || throw(DimensionMismatch("front must be n_front x M"))
    F = Matrix{Float64}(front); μ = Matrix{Float64}(mu); σ² = Matrix{Float64}(var); R = size(μ, 1); r = _mom_ref(ref, M)
    vals = Vector{Float64}(undef, R); best = Ref(Best(-Inf, -1))
    if want_grad
        dμ = Matrix{Float64}(undef, R, M); dσ² = Matrix{Float64}(undef, R, M)
        check(c_mom_ehvi_values(gp_handle(m), M, F, size(F, 1), r, μ, σ², R, vals, dμ, dσ², best))
        return vals, dμ, dσ², best[].val, Int(best[].idx) + 1
    end
    check(c_mom_ehvi_values(gp_handle(m), M, F, size(F, 1), r, μ, σ², R, vals, C_NULL, C_NULL, best))
    vals, nothing, nothing, best[].val, Int(best[].idx) + 1
end

"""
    score_mom(objs, front, ref, X; want_grad = false)
        -> (scores, grad, mu, var, best value, 1-based best column (0: nothing could win))

An extension: the exact expected hypervolume improvement of the posteriors of the 2 to 4 models `objs` over `front` (n_front x M)
above `ref`, over the columns of X in ONE library call.  `grad` (d x R) is `nothing` without `want_grad`; `mu`, `var` are R x M.
The models live on one device and share the dimension; a model may repeat.
"""
function score_mom(objs::AbstractVector{<:AbstractBOHipModel}, front::AbstractMatrix, ref, X::AbstractMatrix; want_grad::Bool = false)
    M = length(objs)
    2 <= M <= MOM_OBJ_MAX || throw(DimensionMismatch("score_mom takes 2 to $MOM_OBJ_MAX models"))
    size(front, 2) == M || throw(DimensionMismatch("front must be n_front x M"))
    F = Matrix{Float64}(front); r = _mom_ref(ref, M)
    Xc = _cols(objs[1], X); R = size(Xc, 2); d = size(Xc, 1)
    sc = Vector{Float64}(undef, R); μ = Matrix{Float64}(undef, R, M); σ² = Matrix{Float64}(undef, R, M); best = Ref(Best(-Inf, -1))
    g = want_grad ? Matrix{Float64}(undef, d, R) : nothing
    hs = convert(Vector{Ptr{Cvoid}}, map(gp_handle, objs))
    GC.@preserve objs check(c_gp_score_mom(hs, M, F, size(F, 1), r, Xc, R, sc, want_grad ? g : C_NULL, μ, σ², best))
    sc, g, μ, σ², best[].val, Int(best[].idx) + 1
end
