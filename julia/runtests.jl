# runtests.jl -- SURVEY.md row N4 as ONE command, for whoever has Julia, jbrea/BayesianOptimization.jl and an MI355X:
#
#     BOHIP_LIB=/path/to/libbohip.so julia --project=julia julia/runtests.jl
#
# It (1) re-runs the checks of the reference's own test files with the device model (BOHipGPE) substituted for the
# GaussianProcesses.jl model -- each testset names the reference file:line whose assertion it restates -- and, beside every
# device model, (2) builds the SAME model with the reference's own `GPE` / `ElasticGPE` and compares posterior, scores and
# arg-max between the two: that comparison is what turns "parity unpinned" (DESIGN.md section 7) into pinned, and
# (3) writes tests/golden/julia_outputs.txt through gen_golden.jl so the Python suite (tests/test_julia_golden.py) can hold
# the oracle and the device against the real package from then on.
#
# STATUS: never executed -- there is no Julia toolchain in the build image or on the GPU box (INTEGRATION.md section 3).
using Test, Random, LinearAlgebra
using BayesianOptimization, GaussianProcesses
const BO = BayesianOptimization
include(joinpath(@__DIR__, "BOHip.jl"))
using .BOHip

# the synthetic objective of the reference's tests (test/branin.jl:1-5)
branin(x1, x2; a = 1, b = 5.1 / (4π^2), c = 5 / π, r = 6, s = 10, t = 1 / (8π)) =
    a * (x2 - b * x1^2 + c * x1 - r)^2 + s * (1 - t) * cos(x1) + s
branin(x::AbstractVector) = branin(x[1], x[2])
const BRANIN_MINIMA = ([-π, 12.275], [π, 2.275], [9.42478, 2.475])
const BRANIN_FMIN = 0.397887

# relative agreement asked of device vs reference package (BASELINE.json north_star: mu / sigma^2 / EI within 1e-6 rel;
# sigma^2 = s_f^2 - v'v cancels near observations, hence the absolute floor -- SURVEY.md section 7)
close_rel(a, b; rel = 1e-6, floor = 0.0) = all(abs.(a .- b) .<= rel .* abs.(b) .+ floor)

@testset "BOHip vs jbrea/BayesianOptimization.jl" begin

    @testset "acquisition: MaxMean on a one-observation GP peaks at the observation (test/acquisition.jl:1-12)" begin
        ref = GPE(reshape([1.0], 1, 1), [2.0], MeanZero(), SEIso(1.0, 0.0))
        dev = BOHipGPE(reshape([1.0], 1, 1), [2.0]; kernel = :SEIso, loglen = [1.0], logsig = 0.0, logNoise = ref.logNoise.value)
        ac = BO.MaxMean()
        opts = merge(BO.defaultoptions(typeof(dev), typeof(ac)), (maxtime = 3.0,))
        @test opts.maxeval == 2000                                      # :7 (the default the reference asserts on its NLopt object)
        maxf, maxx = BO.acquire_max(ac, dev, [-5.0], [5.0], merge(opts, (restarts = 10,)))
        @test maxx ≈ [1.0] atol = 1e-6                                  # :12
        xs = reshape(collect(range(-5, 5, length = 201)), 1, :)
        μr, σr = BO.mean_var(ref, xs); μd, σd = BO.mean_var(dev, xs)
        @test close_rel(μd, μr) && close_rel(σd, σr; floor = 64 * eps())
    end

    @testset "acquisition functions: batched == single, bit for bit (test/acquisitionfunctions.jl:1-12)" begin
        Random.seed!(1)
        X = rand(3, 4); y = rand(4); x = rand(3, 2)
        ref = GPE(X, y, MeanZero(), SEIso(0.0, 0.0))
        dev = BOHipGPE(X, y; kernel = :SEIso, loglen = [0.0], logsig = 0.0, logNoise = ref.logNoise.value)
        for ac in (ProbabilityOfImprovement(), ExpectedImprovement(), UpperConfidenceBound(), ThompsonSamplingSimple(), MutualInformation())
            fd = BO.acquisitionfunction(ac, dev)
            v = fd(x)
            @test length(v) == 2                                         # :8
            if !(ac isa ThompsonSamplingSimple)
                @test v[1] == fd(x[:, 1])                                # :10 (bit-exact, also on the device)
                fr = BO.acquisitionfunction(ac, ref)
                @test close_rel(v, fr(x); floor = 1e-12)                  # device vs the reference package itself
            end
        end
    end

    @testset "LogEI (an extension): log of the textbook EI, same arg-max, device functor == host functor" begin
        Random.seed!(2)
        X = rand(3, 30); y = vec(sum(sin.(3 .* X), dims = 1)); xs = rand(3, 50)
        dev = BOHipGPE(X, y; kernel = :SEArd, loglen = fill(log(0.5), 3), logsig = 0.0, logNoise = -2.0)
        ac = LogExpectedImprovement(); BO.setparams!(ac, dev)
        @test ac.τ == maximum(y)
        μ, σ² = BO.mean_var(dev, xs)
        v = BO.acquisitionfunction(ac, dev)(xs)
        @test close_rel(v, ac.(μ, σ²); floor = 1e-12)
        z = (μ .- ac.τ) ./ sqrt.(σ²)
        ei = (μ .- ac.τ) .* (0.5 .* BOHip.erfc_.(-z ./ sqrt(2))) .+ sqrt.(σ²) .* exp.(-0.5 .* z .^ 2) ./ sqrt(2π)
        @test argmax(v) == argmax(ei)
        vd, dm, dv = BOHip.acq_eval(ac, μ, σ²)
        @test vd == v && all(dm .> 0) && all(dv .> 0)
    end

    @testset "warm start bookkeeping (test/warmstart.jl:9-70)" begin
        Random.seed!(7)
        ac = ExpectedImprovement()
        x0 = rand(2, 10) * 15.0 .- [5.0; 0.0]
        y0 = -1 .* [branin(x0[:, i]) for i in 1:size(x0, 2)]
        mkmodel() = BOHipGPE(2; mean = -10.0, kernel = :SEArd, loglen = [0.0, 0.0], logsig = 5.0, logNoise = -2.0, capacity = 3000)
        mopt() = MAPGPOptimizer(every = 50, noisebounds = [-4, 3], kernbounds = [[-1, -1, 0], [4, 4, 10]], maxeval = 40)
        # :9-27 initial sampling is tracked
        opt = BOpt(branin, mkmodel(), ac, mopt(), [-5.0, 0.0], [10.0, 15.0]; maxiterations = 10, sense = Min, verbosity = Silent,
                   initializer_iterations = 10)
        boptimize!(opt)
        @test opt.observed_optimum == Int(opt.sense) * maximum(opt.model.y)   # :26
        @test length(opt.model.y) == 10                                       # :27
        # :30-46 a pre-made model is taken over
        pre = mkmodel(); BO.update!(pre, x0, y0)
        opt = BOpt(branin, pre, ac, mopt(), [-5.0, 0.0], [10.0, 15.0]; maxiterations = 10, sense = Min, verbosity = Silent,
                   initializer_iterations = 5)
        @test opt.observed_optimum == Int(opt.sense) * maximum(y0)            # :44
        @test opt.observed_optimizer == x0[:, argmax(y0)]                     # :45
        # :48-70 zero initial iterations on a pre-made model, then five more
        ac = ExpectedImprovement()
        opt = BOpt(branin, pre, ac, mopt(), [-5.0, 0.0], [10.0, 15.0]; maxiterations = 0, sense = Min, verbosity = Silent,
                   initializer_iterations = 0)
        boptimize!(opt)
        @test opt.acquisition.τ == maximum(y0)                                # :64
        @test length(opt.model.x) == length(x0) && length(opt.model.y) == length(y0)   # :65-66
        opt.iterations.N = 5
        boptimize!(opt)
        @test length(opt.model.y) == length(y0) + 5                          # :70
    end

    @testset "branin regret (test/branin.jl:19-37)" begin
        Random.seed!(123)
        for ac in (ProbabilityOfImprovement(), ExpectedImprovement(), UpperConfidenceBound(), ThompsonSamplingSimple(), MutualInformation())
            opt = BOpt(branin, BOHipGPE(2; mean = -10.0, kernel = :SEArd, loglen = [0.0, 0.0], logsig = 5.0, logNoise = -2.0, capacity = 3000),
                       ac, MAPGPOptimizer(every = 50, noisebounds = [-4, 3], kernbounds = [[-1, -1, 0], [4, 4, 10]], maxeval = 40),
                       [-5.0, 0.0], [10.0, 15.0]; maxiterations = 200, sense = Min, verbosity = Silent)
            boptimize!(opt)
            @test abs(opt.observed_optimum - BRANIN_FMIN) < 0.05              # :36
        end
    end

    @testset "device model vs ElasticGPE at BASELINE configs[1] shape (N = 3000, d = 8, R = 4096)" begin
        Random.seed!(0)
        N, d, R = 3000, 8, 4096
        X = rand(d, N); y = vec(sum(sin.(3 .* X), dims = 1)) .+ 0.1 .* randn(N)
        Xs = rand(d, R)
        ref = ElasticGPE(d, mean = MeanConst(0.0), kernel = SEArd(fill(log(0.5), d), 0.0), logNoise = -2.0, capacity = N)
        append!(ref, X, y)
        dev = BOHipGPE(d; mean = 0.0, kernel = :SEArd, loglen = fill(log(0.5), d), logsig = 0.0, logNoise = -2.0, capacity = N)
        BO.update!(dev, X, y)
        μr, σr = BO.mean_var(ref, Xs); μd, σd = BO.mean_var(dev, Xs)
        @test close_rel(μd, μr; floor = 64 * eps() * sum(abs, ref.alpha))
        @test close_rel(σd, σr; floor = 64 * N * eps())
        ac = ExpectedImprovement(); BO.setparams!(ac, ref)
        fr = BO.acquisitionfunction(ac, ref)(Xs)
        sd, fbest, jbest = BOHip.score(dev, ac, Xs)
        @test close_rel(sd, fr; floor = 1e-12)
        @test jbest == findfirst(==(maximum(fr)), fr)                        # arg-max index: first maximum wins (src/acquisition.jl:62)
    end

    @testset "replicated sites (BOHipRep.jl, an extension): 5 evaluations a position as one weighted site == the reference with every column" begin
        Random.seed!(5)
        d, n, r, R = 2, 40, 5, 64
        P = rand(d, n); X = repeat(P, inner = (1, r)); y = vec(sum(sin.(3 .* X), dims = 1)) .+ 0.1 .* randn(n * r)
        Xs = rand(d, R)
        ref = ElasticGPE(d, mean = MeanConst(0.0), kernel = SEArd(fill(log(0.5), d), 0.0), logNoise = -2.0, capacity = n * r)
        append!(ref, X, y)
        dev = BOHipGPE(d; mean = 0.0, kernel = :SEArd, loglen = fill(log(0.5), d), logsig = 0.0, logNoise = -2.0, capacity = n)
        xs, ybar, reps, ss, ymax = BOHip.collapse_evaluations(X, y)
        @test size(xs) == (d, n) && all(reps .== r) && xs == P
        BOHip.append_sites!(dev, xs, ybar, reps, ss, ymax)
        @test BOHip.sites_info(dev)[1:2] == (n, n * r) && BOHip.site_reps(dev) == reps
        @test BO.maxy(dev) == maximum(y)
        μr, σr = BO.mean_var(ref, Xs); μd, σd = BO.mean_var(dev, Xs)
        @test close_rel(μd, μr; floor = 64 * eps() * sum(abs, ref.alpha))
        @test close_rel(σd, σr; floor = 64 * n * r * eps())
        @test isapprox(BOHip.mll(dev), ref.mll; rtol = 1e-9)                  # the likelihood of ALL evaluations
    end
end

# (3) pin the Python oracle against the real package: tests/golden/julia_inputs.txt -> tests/golden/julia_outputs.txt
include(joinpath(@__DIR__, "gen_golden.jl"))
