# BOHipFit.jl -- the batched marginal likelihood (include/bohip_fit.h, DESIGN.md 6i); included by BOHip.jl, inside its module.
# Binds exactly the symbols of that header (checked mechanically in tests/test_fit_host.py, as BOHip.jl is against bohip.h).
c_gp_mll_batch_dims(h, P, nmax) = ccall((:bohip_gp_mll_batch_dims, libbohip), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), h, P, nmax)
c_gp_mll_grad_batch(h, H, theta, mll, grad, pivot) = ccall((:bohip_gp_mll_grad_batch, libbohip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), h, H, theta, mll, grad, pivot)
"""
    mll_batch_dims(m) -> (P, nmax)

Length of one hyper-parameter setting of `mll_grad_batch` and the largest model its batched form takes.
"""
function mll_batch_dims(m::AbstractBOHipModel)
    P = Ref(Int64(0)); nmax = Ref(Int64(0))
    check(c_gp_mll_batch_dims(gp_handle(m), P, nmax))
    Int(P[]), Int(nmax[])
end
"""
    mll_grad_batch(m, Theta; grad = true) -> (mll, G or nothing, pivot)

The log marginal likelihood of the model, and its gradient, at the H COLUMNS of `Theta` (P x H, a column = GP.get_params order with
everything on: [logNoise, mean, ll..., logsig], src/models/gp.jl:55-58) in one launch: the objective of `optimizemodel!`
(src/models/gp.jl:54-77) at many points at once.  `G` is P x H.  A column whose factorisation fails has `pivot > 0` (the 1-based
pivot), `mll = -Inf` and a zero gradient; the call itself succeeds.  The model is not changed.  On a device list the first replica
evaluates.  (A multi-start `optimizemodel!` is not provided here: NLopt runs are sequential.)
"""
function mll_grad_batch(m::AbstractBOHipModel, Theta::AbstractMatrix; grad::Bool = true)
    P, _ = mll_batch_dims(m)
    Tc = Matrix{Float64}(Theta); H = size(Tc, 2)            # P x H column-major = the library's H rows of P
    size(Tc, 1) == P || throw(DimensionMismatch("Theta must be $(P) x H"))
    mll = Vector{Float64}(undef, H); G = grad ? Matrix{Float64}(undef, P, H) : nothing
    pivot = Vector{Int64}(undef, H)
    check(c_gp_mll_grad_batch(gp_handle(m), H, Tc, mll, grad ? G : C_NULL, pivot))
    mll, G, pivot
end
