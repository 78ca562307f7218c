# BOHipKG.jl -- the knowledge gradient over a candidate set, exact, on the device (include/bohip_kg.h, DESIGN.md 6l); included by
# BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked mechanically in tests/test_kg_host.py).
c_gp_kg(h, Xs, R, E, kg, nseg, mu, best) = ccall((:bohip_gp_kg, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Best}), h, Xs, R, E, kg, nseg, mu, best)
c_kg_lines(h, a, B, R, E, kg, nseg) = ccall((:bohip_kg_lines, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Ptr{Int32}), h, a, B, R, E, kg, nseg)
const KG_RMAX = 8192                # BOHIP_KG_RMAX

"""
    kg(m, X; n_eval = size(X, 2)) -> (values, nseg, mu, best value, 1-based best column (0: nothing could win))

An extension (the reference has no such acquisition): the knowledge gradient of the first `n_eval` columns of X over the candidate
set X, KG(e) = E[max_j mu'_j] - max_j mu_j, the expected rise of the maximum of the posterior mean over the candidates after ONE
noisy observation at column e -- computed exactly, by a march along the upper envelope of the lines a_j + b_j Z,
b_j = Sigma_je / sqrt(Sigma_ee + nu).  The posterior covariance stays on the device.  The model is not changed.  On a device list
the first replica runs it.
"""
function kg(m::AbstractBOHipModel, X::AbstractMatrix; n_eval::Integer = size(X, 2))
    Xc = _cols(m, X); R = size(Xc, 2)
    vals = zeros(Float64, max(n_eval, 1)); nseg = zeros(Int32, max(n_eval, 1)); μ = Vector{Float64}(undef, R)
    best = Ref(Best(-Inf, -1))
    check(c_gp_kg(gp_handle(m), Xc, R, n_eval, vals, nseg, μ, best))
    vals, nseg, μ, best[].val, Int(best[].idx) + 1
end
"""
    kg_lines(m, a, B) -> (values, nseg)

The march of `kg` alone on the caller's lines: a holds the R intercepts, B is R x E with the slopes of evaluation point e in COLUMN e
(the library's E x R row-major).  The model supplies the device and the stream only.
"""
function kg_lines(m::AbstractBOHipModel, a::AbstractVector, B::AbstractMatrix)
    ac = Vector{Float64}(a); Bc = Matrix{Float64}(B); R, E = size(Bc)
    R == length(ac) || throw(DimensionMismatch("B must be length(a) x E"))
    vals = zeros(Float64, max(E, 1)); nseg = zeros(Int32, max(E, 1))
    check(c_kg_lines(gp_handle(m), ac, Bc, R, E, vals, nseg))
    vals, nseg
end

"""
    KnowledgeGradient()

The knowledge gradient as an acquisition: a candidate-set acquisition without parameters and without a gradient.  `acquire_max`
takes `maxeval` Latin-hypercube candidates per restart, evaluates each against the whole set in one `kg` call and keeps the first
maximum over the restarts (strict `>`); `method` is accepted and not used.
"""
struct KnowledgeGradient <: AbstractAcquisition end
setparams!(::KnowledgeGradient, model) = nothing
function defaultoptions(::Type{<:AbstractBOHipModel}, ::Type{KnowledgeGradient})
    (method = :LD_LBFGS, restarts = 1, maxeval = 1024)            # 1024: the smallest candidate chunk a model can have
end
function acquire_max_device(::KnowledgeGradient, m::AbstractBOHipModel, lowerbounds, upperbounds, options)
    _check_options(options)
    lb = Float64.(lowerbounds); ub = Float64.(upperbounds)
    maxf = -Inf; maxx = lb
    isempty(m.y) && return maxf, maxx
    for _ in 1:options.restarts
        cand = BO.latin_hypercube_sampling(lb, ub, max(options.maxeval, 1))
        _, _, _, f, j = kg(m, cand)
        if j >= 1 && f > maxf                                     # src/acquisition.jl:62 strict '>'
            maxf = f; maxx = cand[:, j]
        end
    end
    maxf, maxx
end
