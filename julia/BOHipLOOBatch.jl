# BOHipLOOBatch.jl -- the batched leave-one-out objective (include/bohip_loo_batch.h, DESIGN.md 6s); included by BOHip.jl, inside
# its module.  Binds exactly the symbol of that header (checked mechanically in tests/test_loo_batch_host.py).
c_gp_loo_grad_batch(h, H, theta, total, grad, logp, pivot) = ccall((:bohip_gp_loo_grad_batch, libbohip), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), h, H, theta, total, grad, logp, pivot)
"""
    loo_grad_batch(m, Theta; grad = true, logp = false) -> (total, G or nothing, pivot[, logp])

The leave-one-out predictive log-probability of the model (`loo_grad`), and its gradient, at the H COLUMNS of `Theta` (P x H, a
column = [logNoise, mean, ll..., logsig] as for `mll_grad_batch`) in one launch.  `G` is P x H; with `logp = true` the N x H
per-point log-probabilities come back as a fourth value.  A column whose factorisation fails has `pivot > 0` (the 1-based pivot),
`total = -Inf`, a zero gradient and a NaN column of `logp`; the call itself succeeds.  The model is not changed.  At most
`mll_batch_dims(m)[2]` observations.  On a device list the first replica evaluates.
"""
function loo_grad_batch(m::AbstractBOHipModel, Theta::AbstractMatrix; grad::Bool = true, logp::Bool = false)
    P, _ = mll_batch_dims(m)
    Tc = Matrix{Float64}(Theta); H = size(Tc, 2)            # P x H column-major = the library's H rows of P
    size(Tc, 1) == P || throw(DimensionMismatch("Theta must be $(P) x H"))
    total = Vector{Float64}(undef, H); G = grad ? Matrix{Float64}(undef, P, H) : nothing
    lp = logp ? Matrix{Float64}(undef, length(m.y), H) : nothing
    pivot = Vector{Int64}(undef, H)
    check(c_gp_loo_grad_batch(gp_handle(m), H, Tc, total, grad ? G : C_NULL, logp ? lp : C_NULL, pivot))
    logp ? (total, G, pivot, lp) : (total, G, pivot)
end
