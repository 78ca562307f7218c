# BOHipQEHVI.jl -- greedy Monte-Carlo q-EHVI batch selection for two objectives over joint draws on the device
# (include/bohip_qehvi.h, DESIGN.md 6ab); included by BOHip.jl, inside its module.  Binds exactly the symbols of that header (checked
# mechanically in tests/test_qehvi_host.py).  Not run: written against the header.
c_mo_qehvi_select(h, F0, F1, S, R, front, nf, ref, q, idx, gain) = ccall((:bohip_mo_qehvi_select, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}), h, F0, F1, S, R, front, nf, ref, q, idx, gain)
c_gp_qehvi_batch(h0, h1, front, nf, ref, Xs, R, S, seed, jitter, max_tries, q, idx, gain, samples, jused, tused) = ccall((:bohip_gp_qehvi_batch, libbohip), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, UInt64, Float64, Cint, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}), h0, h1, front, nf, ref, Xs, R, S, seed, jitter, max_tries, q, idx, gain, samples, jused, tused)
"""
    qehvi_batch(m0, m1, front, ref, X, q; S = 256, seed = 0, jitter = 1e-12, max_tries = 40)
        -> (1-based columns (0: nothing could win), gains, jitter[2], tries[2])

An extension: q columns of X chosen greedily by Monte-Carlo q-EHVI over S joint posterior draws of each of the two models (both
objectives MAXIMISED), which stay on the device.  `front` is n x 2 (one point per ROW, ascending in the first objective: the
library's 2 x n row-major), `ref` the reference point.  `sum(gains)` is the q-EHVI estimate of the batch.  The models are not changed.
"""
function qehvi_batch(m0::AbstractBOHipModel, m1::AbstractBOHipModel, front::AbstractMatrix, ref::AbstractVector, X::AbstractMatrix,
                     q::Integer; S::Integer = 256, seed::Integer = 0, jitter::Real = 1e-12, max_tries::Integer = 40)
    Xc = _cols(m0, X); R = size(Xc, 2)
    fr = Matrix{Float64}(front); rf = Vector{Float64}(ref)
    idx = fill(Int64(-1), max(q, 1)); gain = zeros(Float64, max(q, 1))
    jused = zeros(Float64, 2); tused = zeros(Cint, 2)
    check(c_gp_qehvi_batch(gp_handle(m0), gp_handle(m1), fr, size(fr, 1), rf, Xc, R, S, UInt64(seed), Float64(jitter), Cint(max_tries), q,
                           idx, gain, C_NULL, jused, tused))
    idx .+ 1, gain, jused, Int.(tused)
end
"""
    qehvi_select(m, F0, F1, front, ref, q) -> (1-based columns (0: nothing could win), gains)

The selection of `qehvi_batch` alone on the caller's draws: F0 and F1 are R x S, one draw per COLUMN (the library's S x R row-major).
The model supplies the device and the stream only.
"""
function qehvi_select(m::AbstractBOHipModel, F0::AbstractMatrix, F1::AbstractMatrix, front::AbstractMatrix, ref::AbstractVector, q::Integer)
    A = Matrix{Float64}(F0); B = Matrix{Float64}(F1); R, S = size(A)
    fr = Matrix{Float64}(front); rf = Vector{Float64}(ref)
    idx = fill(Int64(-1), max(q, 1)); gain = zeros(Float64, max(q, 1))
    check(c_mo_qehvi_select(gp_handle(m), A, B, S, R, fr, size(fr, 1), rf, q, idx, gain))
    idx .+ 1, gain
end
