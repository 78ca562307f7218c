# BOHipNEIGrad.jl -- the gradient of noisy expected improvement in the candidate, on the device (include/bohip_nei_grad.h, DESIGN.md 6x);
# included by BOHip.jl, inside its module, after BOHipNEI.jl.  Binds exactly the symbol of that header (checked mechanically in
# tests/test_nei_grad_host.py).
c_gp_score_nei_grad(h, acq, prm, Xs, R, S, seed, jrel, sc, grad, mu, var, best) = ccall((:bohip_gp_score_nei_grad, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, prm, Xs, R, S, seed, jrel, sc, grad, mu, var, best)

"""
    nei_grad(m, X; S = 32, seed = 0, acq = :ei, jitter_rel = 1e-8) -> (score, grad, mu, var, best value, 1-based best column, tau)

An extension, beside `nei`: noisy expected improvement at the columns of `X` and its gradient with respect to every candidate,
grad[:, j] = d NEI(x_j) / dx (d x R, as `score_grad`).  With `seed` fixed the score is one deterministic function of x: what an
L-BFGS ascent climbs.  `score`, `mu` and `var` agree with `nei`'s to rounding.  On a device list the first replica runs it.  The model
is not changed.
"""
function nei_grad(m::AbstractBOHipModel, X::AbstractMatrix; S::Integer = 32, seed::Integer = 0, acq::Symbol = :ei, jitter_rel::Real = 1e-8)
    haskey(NEI_ACQ, acq) || throw(ArgumentError("acq must be :ei, :pi or :logei"))
    Xc = _cols(m, X); R = size(Xc, 2); d = size(Xc, 1)
    sc = Vector{Float64}(undef, R); mu = similar(sc); var = similar(sc); tau = Vector{Float64}(undef, max(S, 1))
    g = Matrix{Float64}(undef, d, R)
    best = Ref(Best(-Inf, -1))
    check(c_gp_nei_fantasies(gp_handle(m), Float64(jitter_rel), S, UInt64(seed), C_NULL, tau))
    check(c_gp_score_nei_grad(gp_handle(m), NEI_ACQ[acq], C_NULL, Xc, R, S, UInt64(seed), Float64(jitter_rel), sc, g, mu, var, best))
    sc, g, mu, var, best[].val, Int(best[].idx) + 1, tau
end
