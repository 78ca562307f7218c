# BOHipPend.jl -- pending evaluations (include/bohip_pend.h, DESIGN.md 6u); included by BOHip.jl, inside its module.  Binds exactly the
# symbols of that header (checked mechanically in tests/test_pend_host.py).  Like the rest of the binding it has never been executed:
# there is no Julia toolchain where the library is built; the functions restate the Python host layer
# (bayesianoptimization.jl_amd/model.py, acquisition.py) statement for statement.
c_gp_pending_set(h, Xp, p) = ccall((:bohip_gp_pending_set, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h, Xp, p)
c_gp_pending_info(h, p, Xp, mu, cov) = ccall((:bohip_gp_pending_info, libbohip), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, p, Xp, mu, cov)
c_gp_score_pending(h, acq, prm, Xs, R, S, seed, flags, sc, mu, var, best) = ccall((:bohip_gp_score_pending, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, prm, Xs, R, S, seed, flags, sc, mu, var, best)
c_pend_values(h, acq, prm, R, p, S, mu, var, B, Z, tau, sc, best) = ccall((:bohip_pend_values, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, prm, R, p, S, mu, var, B, Z, tau, sc, best)

const PEND_PMAX = 32        # BOHIP_PEND_PMAX
const PEND_SMAX = 1024      # BOHIP_PEND_SMAX
const PEND_RAISE_TAU = Cint(1)

"""
    pending_set!(m::BOHipGPE, Xp) -> m

The points that are out for evaluation and not back yet (d x p, p <= $PEND_PMAX; an empty matrix clears the set).  Nothing is computed
until `score_pending` or `pending_info` reads the set; every other function ignores it.
"""
function pending_set!(m::BOHipGPE, Xp::AbstractMatrix)
    X = Matrix{Float64}(Xp)
    size(X, 2) == 0 || size(X, 1) == m.dim || throw(DimensionMismatch("expected $(m.dim) rows (one point per column)"))
    check(c_gp_pending_set(m.handle, size(X, 2) == 0 ? C_NULL : X, size(X, 2)))
    m
end
pending_set!(m::BOHipMultiGPE, Xp) = throw(ArgumentError("BOHipMultiGPE does not support pending evaluations: they run on one device"))

"(Xp d x p, mu_p, Sigma_p): the pending set with the model's predictive mean and covariance of the noisy outcomes there."
function pending_info(m::BOHipGPE)
    p = Ref{Int64}(0)
    check(c_gp_pending_info(m.handle, p, C_NULL, C_NULL, C_NULL))
    Xp = Matrix{Float64}(undef, m.dim, p[]); mu = Vector{Float64}(undef, p[]); cov = Matrix{Float64}(undef, p[], p[])
    p[] > 0 && check(c_gp_pending_info(m.handle, C_NULL, Xp, mu, cov))
    Xp, mu, cov
end

"""
    score_pending(m, a, X; fantasies = 0, seed = 0, raise_tau = false) -> (scores, mu, var, best value, 1-based best column)

The acquisition `a` averaged over `fantasies` fantasised outcomes at the pending points (bohip_gp_score_pending; Snoek, Larochelle &
Adams 2012, section 3.2); 0 fantasies: the Kriging believer.  `mu` is the model's mean, `var` the variance conditioned on the pending
points.  With an empty pending set it is `score`.  The model is not changed.
"""
function score_pending(m::BOHipGPE, a::AbstractAcquisition, X::AbstractMatrix; fantasies::Integer = 0, seed::Integer = 0, raise_tau::Bool = false)
    Xc = _cols(m, X); R = size(Xc, 2)
    sc = Vector{Float64}(undef, R); mu = similar(sc); var = similar(sc)
    best = Ref(Best(-Inf, -1))
    check(c_gp_score_pending(m.handle, acqid(a), acqparams(a), Xc, R, fantasies, UInt64(seed), raise_tau ? PEND_RAISE_TAU : Cint(0), sc, mu, var, best))
    sc, mu, var, best[].val, Int(best[].idx) + 1
end

"""
    acquire_max_pending(a, m, lowerbounds, upperbounds; restarts = 10, maxeval = 2000, fantasies = 16, raise_tau = true) -> (maxf, maxx)

`restarts` Latin-hypercube candidate sets of `maxeval` points, each scored by ONE `score_pending` call whose seed is drawn after the
candidates; the first maximum wins (strict `>`).  There is no gradient in x.  The caller has run `setparams!`.
"""
function acquire_max_pending(a::AbstractAcquisition, m::BOHipGPE, lowerbounds, upperbounds; restarts::Integer = 10, maxeval::Integer = 2000,
                             fantasies::Integer = 16, raise_tau::Bool = true)
    maxf = -Inf; maxx = Vector{Float64}(lowerbounds)
    for _ in 1:restarts
        X = BO.latin_hypercube_sampling(lowerbounds, upperbounds, max(maxeval, 1))
        seed = rand(UInt64) >> 1
        _, _, _, f, j = score_pending(m, a, X; fantasies = fantasies, seed = seed, raise_tau = raise_tau)
        if j > 0 && f > maxf
            maxf = f; maxx = X[:, j]
        end
    end
    maxf, maxx
end
