# BOHipLOO.jl -- leave-one-out cross-validation of the resident model (include/bohip_loo.h, DESIGN.md 6r); included by BOHip.jl,
# inside its module.  Binds exactly the symbols of that header (checked mechanically in tests/test_loo_host.py).
c_gp_loo(h, mu, var, logp, total) = ccall((:bohip_gp_loo, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, mu, var, logp, total)
c_gp_loo_grad(h, total, dn, dm, dk) = ccall((:bohip_gp_loo_grad, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, total, dn, dm, dk)
"""
    loo(m) -> (μ, σ², logp, total, z)

Leave-one-out predictions of the model at its observations (GaussianProcesses.jl `predict_LOO`, `logp_LOO`): the mean and variance
of every noisy `y[i]` given all the others, its log-probability, their sum, and the standardised residuals
`z = (y .- μ) ./ sqrt.(σ²)` of Jones, Schonlau & Welch 1998.  One pass over the resident inverse factor; the model is not changed.
On a device list the first replica evaluates.
"""
function loo(m::AbstractBOHipModel)
    n = length(m.y)
    μ = Vector{Float64}(undef, n); σ² = Vector{Float64}(undef, n); logp = Vector{Float64}(undef, n); total = Ref(0.0)
    check(c_gp_loo(gp_handle(m), μ, σ², logp, total))
    μ, σ², logp, total[], (m.y .- μ) ./ sqrt.(σ²)
end
"""
    loo_grad(m) -> (total, dlogNoise, dmean, dkern)

The leave-one-out predictive log-probability and its gradient (GaussianProcesses.jl `dlogpdθ_LOO`; Rasmussen & Williams 5.4.2) in
the parameter order of `GaussianProcesses.get_params`: `dkern = [dll..., dlogsig]`, one length entry for an iso kernel.
"""
function loo_grad(m::AbstractBOHipModel)
    nk = length(m.loglen) + 1
    total = Ref(0.0); dn = Ref(0.0); dm = Ref(0.0); dk = Vector{Float64}(undef, nk)
    check(c_gp_loo_grad(gp_handle(m), total, dn, dm, dk))
    total[], dn[], dm[], dk
end
