# BOHipKGGrad.jl -- the knowledge gradient at free points over a resident discretisation, and its gradient in the point
# (include/bohip_kg_grad.h, DESIGN.md 6aa); included by BOHip.jl, inside its module, after BOHipKG.jl.  Binds exactly the symbols of that
# header (checked mechanically in tests/test_kg_grad_host.py); the ccalls only: A is d x R and Xe, grad are d x E, column = point.
c_gp_kg_set_points(h, A, R) = ccall((:bohip_gp_kg_set_points, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h, A, R)
c_gp_kg_points_info(h, what, value, cap) = ccall((:bohip_gp_kg_points_info, libbohip), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64), h, what, value, cap)
c_gp_kg_grad(h, Xe, E, kg, grad, nseg, mu, var, best) = ccall((:bohip_gp_kg_grad, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Best}), h, Xe, E, kg, grad, nseg, mu, var, best)
