# BOHipQEIJoint.jl -- the joint q-EI of B batches of q points and its gradient, on the device (include/bohip_qei_joint.h, DESIGN.md 6z);
# included by BOHip.jl, inside its module, after BOHipQEI.jl.  Binds exactly the symbol of that header (checked mechanically in
# tests/test_qei_joint_host.py); the ccall only: Xs and grad are d x B q, batch b = columns (b - 1) q + 1 .. b q; grad may be C_NULL.
c_gp_qei_joint(h, Xs, B, q, S, seed, tau, jitter_rel, value, grad, mu, pivot) = ccall((:bohip_gp_qei_joint, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, UInt64, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}), h, Xs, B, q, S, seed, tau, jitter_rel, value, grad, mu, pivot)
