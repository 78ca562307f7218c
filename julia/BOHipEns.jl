# BOHipEns.jl -- one acquisition averaged over H hyper-parameter settings, on the device (include/bohip_ens.h, DESIGN.md 6m);
# included by BOHip.jl, inside its module.  Binds exactly the symbol of that header (checked mechanically in tests/test_ens_host.py).
c_gp_score_ens(h, acq, p, H, theta, w, Xs, R, scores, each, mu, var, pivot, best) = ccall((:bohip_gp_score_ens, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Best}), h, acq, p, H, theta, w, Xs, R, scores, each, mu, var, pivot, best)

"""
    score_ensemble(m, a, X, Theta; weights = nothing, each = false, moments = false)
        -> (scores, best value, 1-based best column (0: nothing could win), pivot, each, mu, var)

An extension (the reference scores under its one MAP setting): the acquisition `a` averaged over the hyper-parameter settings in the
COLUMNS of Theta (P x H, a column = [logNoise, mean, ll..., lsigma], `mll_grad_batch`'s layout; the library's H x P row-major):
scores[j] = sum_h w~_h a(x_j; theta_h), the integrated acquisition of Snoek, Larochelle & Adams 2012.  `weights` (H numbers >= 0,
default equal) are renormalised over the settings whose factorisation succeeds; a failed setting has pivot > 0, NaN entries in
`each` / `mu` / `var` (R x H, returned where asked for) and takes no part.  The model itself is neither read beyond its observations
nor changed; at most `mll_batch_dims(m)[2]` observations.  Value only: no gradient.  On a device list the first replica runs it.
"""
function score_ensemble(m::AbstractBOHipModel, a::AbstractAcquisition, X::AbstractMatrix, Theta::AbstractMatrix;
                        weights = nothing, each::Bool = false, moments::Bool = false)
    Xc = _cols(m, X); R = size(Xc, 2)
    Tc = Matrix{Float64}(Theta); H = size(Tc, 2)
    w = weights === nothing ? C_NULL : Vector{Float64}(weights)
    weights === nothing || length(w) == H || throw(DimensionMismatch("weights must have one entry per column of Theta"))
    sc = Vector{Float64}(undef, R); piv = zeros(Int64, H)
    ea = each ? Matrix{Float64}(undef, R, H) : C_NULL
    μ = moments ? Matrix{Float64}(undef, R, H) : C_NULL
    σ² = moments ? Matrix{Float64}(undef, R, H) : C_NULL
    best = Ref(Best(-Inf, -1))
    check(c_gp_score_ens(gp_handle(m), acqid(a), acqparams(a), H, Tc, w, Xc, R, sc, ea, μ, σ², piv, best))
    sc, best[].val, Int(best[].idx) + 1, piv, each ? ea : nothing, moments ? μ : nothing, moments ? σ² : nothing
end
