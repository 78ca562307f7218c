"""The reference's noisy-Branin setting (examples/branin_hartmann.jl of jbrea/BayesianOptimization.jl: Branin with noiselevel = 1,
minimised on [-5, 10] x [0, 15]) under noisy expected improvement, beside ExpectedImprovement at tau = maxy.  Needs an
MI355X.  Prints, for both acquisitions, the regret of the observed optimizer and of the model optimizer; under
NoisyExpectedImprovement the model optimizer is the observed SITE with the largest posterior mean."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import bohip as bo

MINIMA, FMIN = np.array([[-math.pi, 12.275], [math.pi, 2.275], [9.42478, 2.475]]), 0.397887


def branin(x, noiselevel=0.0, rng=None):
    a, b, c, r, s, t = 1.0, 5.1 / (4 * math.pi ** 2), 5 / math.pi, 6.0, 10.0, 1 / (8 * math.pi)
    v = a * (x[1] - b * x[0] ** 2 + c * x[0] - r) ** 2 + s * (1 - t) * math.cos(x[0]) + s
    return v + (noiselevel * float(rng.standard_normal()) if noiselevel else 0.0)


def run(acquisition, seed, iterations=60):
    rng = np.random.default_rng(seed)
    model = bo.ElasticGPE(2, mean=bo.MeanConst(-30.0), kernel=bo.SEArd([1.0, 1.0], 3.0), logNoise=0.0, capacity=iterations + 8)
    opt = bo.BOpt(lambda x: branin(x, 1.0, rng), model, acquisition,
                  bo.MAPGPOptimizer(every=20, noisebounds=[-4, 3], kernbounds=[[-3, -3, -3], [6, 6, 8]], maxeval=40),
                  [-5.0, 0.0], [10.0, 15.0], maxiterations=iterations, sense=bo.Min, verbosity=bo.Silent,
                  acquisitionoptions=dict(restarts=1, maxeval=2048), rng=np.random.default_rng(seed + 1))
    res = bo.boptimize_(opt)
    model.close()
    return branin(res["observed_optimizer"]) - FMIN, branin(res["model_optimizer"]) - FMIN


if __name__ == "__main__":
    for name, make in (("ExpectedImprovement (tau = maxy)", bo.ExpectedImprovement),
                       ("NoisyExpectedImprovement (S = 32)", lambda: bo.NoisyExpectedImprovement(S=32, seed=0))):
        reg = np.array([run(make(), seed) for seed in range(5)])
        print(f"{name:36s} regret of the observed optimizer {reg[:, 0].mean():7.3f}   of the model optimizer {reg[:, 1].mean():7.3f}   (5 runs of 60 evaluations)")
