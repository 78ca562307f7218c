# BOHipQEI.jl -- greedy Monte-Carlo q-EI batch selection over joint draws on the device (include/bohip_qei.h, DESIGN.md 6j);
# included by BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked mechanically in tests/test_qei_host.py).
c_gp_qei_batch(h, Xs, R, S, seed, jitter, max_tries, tau, q, idx, gain, samples, jused, tused) = ccall((:bohip_gp_qei_batch, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, UInt64, Float64, Cint, Float64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}), h, Xs, R, S, seed, jitter, max_tries, tau, q, idx, gain, samples, jused, tused)
c_gp_qei_select(h, samples, S, R, tau, q, idx, gain) = ccall((:bohip_gp_qei_select, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Float64, Int64, Ptr{Int64}, Ptr{Float64}), h, samples, S, R, tau, q, idx, gain)
"""
    qei_batch(m, X, q; S = 256, seed = 0, tau = maxy(m), jitter = 1e-12, max_tries = 40, samples = false)
        -> (1-based columns (0: nothing could win), gains, jitter, tries, samples R x S or nothing)

An extension, as `acquire_batch` is: q columns of X chosen greedily by Monte-Carlo q-EI, qEI(B) = E[max(max_{j in B} f_j - tau, 0)],
over the S joint posterior draws of `sample_joint` for the same (X, S, seed, jitter rule) -- the reference's joint draw
`rand(gp, X)`, src/models/gp.jl:7 -- which stay on the device.  `sum(gains)` is the q-EI estimate of the batch.  With q = 1 it
estimates the textbook EI, Delta Phi(z) + sigma phi(z), not the `ExpectedImprovement` functor's Delta Phi(z) + phi(z).  The model
is not changed.  On a device list the first replica runs it.
"""
function qei_batch(m::AbstractBOHipModel, X::AbstractMatrix, q::Integer; S::Integer = 256, seed::Integer = 0, tau::Real = maxy(m),
                   jitter::Real = 1e-12, max_tries::Integer = 40, samples::Bool = false)
    Xc = _cols(m, X); R = size(Xc, 2)
    idx = fill(Int64(-1), max(q, 1)); gain = zeros(Float64, max(q, 1))
    F = samples ? Matrix{Float64}(undef, R, S) : nothing          # the library's S x R row-major = R x S column-major
    jused = Ref(0.0); tused = Ref(Cint(0))
    check(c_gp_qei_batch(gp_handle(m), Xc, R, S, UInt64(seed), Float64(jitter), Cint(max_tries), Float64(tau), q, idx, gain,
                         samples ? F : C_NULL, jused, tused))
    idx .+ 1, gain, jused[], Int(tused[]), F
end
"""
    qei_select(m, F, tau, q) -> (1-based columns (0: nothing could win), gains)

The selection of `qei_batch` alone on the caller's draws: F is R x S, one draw per COLUMN (the library's S x R row-major).  The
model supplies the device and the stream only.
"""
function qei_select(m::AbstractBOHipModel, F::AbstractMatrix, tau::Real, q::Integer)
    Fc = Matrix{Float64}(F); R, S = size(Fc)
    idx = fill(Int64(-1), max(q, 1)); gain = zeros(Float64, max(q, 1))
    check(c_gp_qei_select(gp_handle(m), Fc, S, R, Float64(tau), q, idx, gain))
    idx .+ 1, gain
end
