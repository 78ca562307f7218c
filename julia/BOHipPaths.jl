# BOHipPaths.jl -- posterior sample paths (include/bohip_paths.h, DESIGN.md 6h); included by BOHip.jl, inside its module.
# Binds exactly the symbols of that header (checked mechanically in tests/test_path_host.py, as BOHip.jl is against bohip.h).
c_gp_paths_draw(h, S, M, seed, out) = ccall((:bohip_gp_paths_draw, libbohip), Cint, (Ptr{Cvoid}, Int64, Int64, UInt64, Ptr{Ptr{Cvoid}}), h, S, M, seed, out)
c_paths_destroy(p) = ccall((:bohip_paths_destroy, libbohip), Cvoid, (Ptr{Cvoid},), p)
c_paths_dims(p, S, M, N, d) = ccall((:bohip_paths_dims, libbohip), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), p, S, M, N, d)
c_paths_eval(p, Xs, R, values, best) = ccall((:bohip_paths_eval, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Best}), p, Xs, R, values, best)
c_paths_eval_grad(p, Xs, R, path_of, f, grad) = ccall((:bohip_paths_eval_grad, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}), p, Xs, R, path_of, f, grad)
c_paths_coef(p, s, omega, w, u) = ccall((:bohip_paths_coef, libbohip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), p, s, omega, w, u)
"""
    draw_paths(m, S; M = 2048, seed = 0) -> BOHipPaths

S posterior SAMPLE PATHS of the model (bohip_gp_paths_draw): draws that are functions, random features for the prior term and the
exact data term (pathwise conditioning).  The object copies what it needs of the model and does not follow its later changes;
`close(paths)` releases it (call it before the model is finalised).  On a device list the first replica holds it.
"""
mutable struct BOHipPaths
    handle::Ptr{Cvoid}
    dim::Int
    S::Int
    M::Int
    N::Int
end
function draw_paths(m::AbstractBOHipModel, S::Integer; M::Integer = 2048, seed::Integer = 0)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(c_gp_paths_draw(gp_handle(m), S, M, UInt64(seed), out))
    h = out[]
    s = Ref(Int64(0)); mm = Ref(Int64(0)); n = Ref(Int64(0)); d = Ref(Int64(0))
    check(c_paths_dims(h, s, mm, n, d))
    BOHipPaths(h, Int(d[]), Int(s[]), Int(mm[]), Int(n[]))
end
function Base.close(p::BOHipPaths)
    p.handle == C_NULL || c_paths_destroy(p.handle)
    p.handle = C_NULL
    nothing
end
"""
    paths_eval(p, X; values = true) -> (values R x S or nothing, best values, 1-based best columns)

Every path at the columns of X, and the arg-max of every path (strict '>', ties -> the smallest column).
"""
function paths_eval(p::BOHipPaths, X::AbstractMatrix; values::Bool = true)
    Xc = Matrix{Float64}(X); R = size(Xc, 2)
    size(Xc, 1) == p.dim || throw(DimensionMismatch("X must be $(p.dim) x R"))
    V = values ? Matrix{Float64}(undef, R, p.S) : nothing         # the library's S x R row-major = R x S column-major
    best = Vector{Best}(undef, p.S)
    check(c_paths_eval(p.handle, Xc, R, values ? V : C_NULL, best))
    V, map(b -> b.val, best), map(b -> Int(b.idx) + 1, best)
end
"""
    paths_eval_grad(p, X; path_of = nothing) -> (f, d x R gradient)

Column j of X on path `path_of[j]` (1-based; nothing: the first path), value and analytic gradient.
"""
function paths_eval_grad(p::BOHipPaths, X::AbstractMatrix; path_of = nothing)
    Xc = Matrix{Float64}(X); R = size(Xc, 2)
    size(Xc, 1) == p.dim || throw(DimensionMismatch("X must be $(p.dim) x R"))
    f = Vector{Float64}(undef, R); g = Matrix{Float64}(undef, p.dim, R)
    po = path_of === nothing ? C_NULL : Vector{Int64}(collect(path_of) .- 1)
    check(c_paths_eval_grad(p.handle, Xc, R, po, f, g))
    f, g
end
"""
    paths_coef(p, s) -> (omega d x F, w, u) of path s (1-based)
"""
function paths_coef(p::BOHipPaths, s::Integer)
    om = Matrix{Float64}(undef, p.dim, p.M ÷ 2); w = Vector{Float64}(undef, p.M); u = Vector{Float64}(undef, p.N)
    check(c_paths_coef(p.handle, s - 1, om, w, u))
    om, w, u
end
