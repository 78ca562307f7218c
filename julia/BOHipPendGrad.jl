# BOHipPendGrad.jl -- the gradient of the acquisition under pending evaluations, on the device (include/bohip_pend_grad.h, DESIGN.md 6y);
# included by BOHip.jl, inside its module, after BOHipPend.jl.  Binds exactly the symbol of that header (checked mechanically in
# tests/test_pend_grad_host.py); the ccall only: grad is d x R as `score_grad` returns it, the other arguments are `c_gp_score_pending`'s.
c_gp_score_pending_grad(h, acq, prm, Xs, R, S, seed, flags, sc, grad, mu, var, best) = ccall((:bohip_gp_score_pending_grad, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, acq, prm, Xs, R, S, seed, flags, sc, grad, mu, var, best)
