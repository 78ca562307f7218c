# BOHipEnsGrad.jl -- the gradient of an acquisition averaged over H hyper-parameter settings, on the device
# (include/bohip_ens_grad.h, DESIGN.md 6n); included by BOHip.jl, inside its module.  Binds exactly the symbol of that header
# (checked mechanically in tests/test_ens_grad_host.py).
c_gp_score_ens_grad(h, acq, p, H, theta, w, Xs, R, scores, grad, each, each_grad, mu, var, pivot, best) = ccall((:bohip_gp_score_ens_grad, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Best}), h, acq, p, H, theta, w, Xs, R, scores, grad, each, each_grad, mu, var, pivot, best)

"""
    score_ensemble_grad(m, a, X, Theta; weights = nothing, each = false)
        -> (scores, grad, best value, 1-based best column (0: nothing could win), pivot, each, each_grad)

An extension, beside `score_ensemble`: the averaged acquisition and its gradient with respect to every candidate,
grad[:, j] = sum_h w~_h d a(x_j; theta_h) / dx (d x R, as `score_grad`).  The scores, `each` (R x H) and the arg-max are those of
`score_ensemble` bit for bit; `each_grad` (d x R x H, where asked for) holds the per-setting gradients, NaN for a failed setting.
Successive calls with the same Theta and unchanged observations factor once (an ascent's calls).  On a device list the first replica
runs it.
"""
function score_ensemble_grad(m::AbstractBOHipModel, a::AbstractAcquisition, X::AbstractMatrix, Theta::AbstractMatrix;
                             weights = nothing, each::Bool = false)
    Xc = _cols(m, X); R = size(Xc, 2); d = size(Xc, 1)
    Tc = Matrix{Float64}(Theta); H = size(Tc, 2)
    w = weights === nothing ? C_NULL : Vector{Float64}(weights)
    weights === nothing || length(w) == H || throw(DimensionMismatch("weights must have one entry per column of Theta"))
    sc = Vector{Float64}(undef, R); piv = zeros(Int64, H)
    g = Matrix{Float64}(undef, d, R)
    ea = each ? Matrix{Float64}(undef, R, H) : C_NULL
    eg = each ? Array{Float64}(undef, d, R, H) : C_NULL
    best = Ref(Best(-Inf, -1))
    check(c_gp_score_ens_grad(gp_handle(m), acqid(a), acqparams(a), H, Tc, w, Xc, R, sc, g, ea, eg, C_NULL, C_NULL, piv, best))
    sc, g, best[].val, Int(best[].idx) + 1, piv, each ? ea : nothing, each ? eg : nothing
end
