# BOHipRep.jl -- replicated sites (include/bohip_rep.h, DESIGN.md 6t); included by BOHip.jl, inside its module.  Binds exactly the symbols
# of that header (checked mechanically in tests/test_rep_host.py).  Like the rest of the binding it has never been executed: there is
# no Julia toolchain where the library is built; `append_sites!` and `collapse_evaluations` restate the Python host layer
# (bayesianoptimization.jl_amd/model.py) statement for statement.
c_gp_append_sites(h, X, ybar, reps, ss, p) = ccall((:bohip_gp_append_sites, libbohip), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Int64), h, X, ybar, reps, ss, p)
c_gp_sites_info(h, n, ne, ss, slr, w) = ccall((:bohip_gp_sites_info, libbohip), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}), h, n, ne, ss, slr, w)
c_gp_get_reps(h, reps) = ccall((:bohip_gp_get_reps, libbohip), Cint, (Ptr{Cvoid}, Ptr{Int64}), h, reps)

# the largest raw evaluation among the sites a model was given (a site's mean is never above it): what maxy adds to maximum(m.y)
const _site_ymax = WeakKeyDict{BOHipGPE, Float64}()
maxy(m::BOHipGPE) = isempty(m.y) ? -Inf : max(maximum(m.y), get(_site_ymax, m, -Inf))

"""
    collapse_evaluations(x, y) -> (x_sites, ybar, reps, ss, ymax)

Repeated evaluations as weighted sites: groups the identical columns of `x` (d x N, compared bit for bit) within this call, in order
of first occurrence, wherever they stand.  `ybar` is the mean of a site's evaluations, `reps` their count, `ss` the within-site sum of
squares `sum((y_j - ybar)^2)` computed in a second pass around the mean (exactly 0 for a single evaluation), `ymax` the largest raw
value.
"""
function collapse_evaluations(x, y)
    X = Matrix{Float64}(x isa AbstractVector ? reshape(x, :, 1) : x); Y = Vector{Float64}(vec(collect(y)))
    size(X, 2) == length(Y) || throw(DimensionMismatch("x and y disagree on the number of observations"))
    seen = Dict{Vector{UInt64}, Int}(); members = Vector{Vector{Int}}()
    for j in 1:length(Y)
        key = collect(reinterpret(UInt64, X[:, j]))
        if !haskey(seen, key)
            seen[key] = length(members) + 1
            push!(members, Int[])
        end
        push!(members[seen[key]], j)
    end
    n = length(members)
    xs = X[:, map(m -> m[1], members)]
    ybar = Vector{Float64}(undef, n); reps = Vector{Int64}(undef, n); ss = Vector{Float64}(undef, n); ymax = Vector{Float64}(undef, n)
    for (i, m) in enumerate(members)
        v = Y[m]
        reps[i] = length(v)
        ybar[i] = length(v) == 1 ? v[1] : sum(v) / length(v)
        ss[i] = length(v) == 1 ? 0.0 : sum((v .- ybar[i]) .^ 2)
        ymax[i] = maximum(v)
    end
    xs, ybar, reps, ss, ymax
end

"""
    append_sites!(m::BOHipGPE, x, ybar, reps, ss, ymax = ybar) -> m

Append weighted sites (`bohip_gp_append_sites`): column j of `x` with the mean `ybar[j]` of its `reps[j]` evaluations and their
within-site sum of squares `ss[j]`.  `m.x` and `m.y` are then site positions and site means; `maxy(m)` stays the largest raw
evaluation.  All `reps == 1` on an unweighted model is `update!`.  A device list takes no sites.
"""
function append_sites!(m::BOHipGPE, x, ybar, reps, ss, ymax = ybar)
    X = Matrix{Float64}(reshape(x, m.dim, :)); Y = Vector{Float64}(vec(collect(ybar)))
    r = Vector{Int64}(vec(collect(reps))); s = Vector{Float64}(vec(collect(ss))); top = Vector{Float64}(vec(collect(ymax)))
    size(X, 2) == length(Y) == length(r) == length(s) == length(top) || throw(DimensionMismatch("x, ybar, reps, ss and ymax disagree on the number of sites"))
    rc = c_gp_append_sites(m.handle, X, Y, r, s, length(Y))
    if rc == 0 || rc == -2                                                                # sites are stored even if the factorisation failed
        m.x = hcat(m.x, X); append!(m.y, Y)
        isempty(top) || (_site_ymax[m] = max(get(_site_ymax, m, -Inf), maximum(top)))
    end
    check(rc)
    m
end
append_sites!(m::BOHipMultiGPE, args...) = throw(ArgumentError("BOHipMultiGPE does not support replicated sites: the device list keeps its replicas in step by plain appends"))

"`update!` of a model that collapses: the repeated columns of the call as one weighted site each."
update_collapsed!(m::BOHipGPE, x, y) = append_sites!(m, collapse_evaluations(reshape(x, m.dim, :), y)...)

"(n_sites, n_evals, sum s_i, sum log r_i, weighted) as the handle keeps them."
function sites_info(m::BOHipGPE)
    n = Ref{Int64}(0); ne = Ref{Int64}(0); ss = Ref(0.0); slr = Ref(0.0); w = Ref{Cint}(0)
    check(c_gp_sites_info(m.handle, n, ne, ss, slr, w))
    n[], ne[], ss[], slr[], w[] != 0
end
"Evaluations behind every row of the model (all 1 unless sites were appended)."
function site_reps(m::BOHipGPE)
    r = Vector{Int64}(undef, length(m.y))
    check(c_gp_get_reps(m.handle, r))
    r
end
