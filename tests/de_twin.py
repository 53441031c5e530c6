"""Host twin of the device differential evolution (sbo_fit_de, csrc/fit.hip) -- test infrastructure for
tests/test_gpu_fit_shapes.py.

A plain restatement of the device algorithm, draw for draw: the counter-based generator (splitmix64's finaliser ``mix64`` and
``u01(seed, gen, member, draw)``), the host's dithered F sequence, the r0 / r1 selection, the binomial crossover with its forced
entry, the out-of-bounds redraw, the deferred ``take = e <= energy[i]`` update and the convergence check every 8th generation
and at the last one.  The energies come from a caller-supplied ``energy(pop) -> [P]`` -- on the device's NLL (the same
``nll_member`` as the DE's own launches, built with -ffp-contract=off) the twin's result is the device's bit for bit."""
import math

import numpy as np

M64 = (1 << 64) - 1
CR = 0.7


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def u01(seed, gen, member, draw):
    k = mix64((seed & M64) ^ mix64(((gen & 0xFFFFFFFF) << 32) | (member & 0xFFFFFFFF)) ^ mix64((0xDA3E39CB94B95BDB + draw) & M64))
    return float(k >> 11) * (1.0 / 9007199254740992.0)


def f_sequence(seed, gens):
    """The mutation factor of each generation: fstate = mix64(seed), then one mix64 per generation, F in [0.5, 1)."""
    out, state = [], mix64(seed & M64)
    for _ in range(gens):
        state = mix64(state)
        out.append(0.5 + 0.5 * (float(state >> 11) * (1.0 / 9007199254740992.0)))
    return out


def select(seed, gen, i, P):
    """r0, r1: two distinct members other than i (the device's draws 0 and 1)."""
    r0 = int(u01(seed, gen, i, 0) * (P - 1))
    r1 = int(u01(seed, gen, i, 1) * (P - 2))
    if r0 >= i:
        r0 += 1
    lo_, hi_ = (r0, i) if r0 < i else (i, r0)
    if r1 >= lo_:
        r1 += 1
    if r1 >= hi_:
        r1 += 1
    return r0, r1


def best_index(energy):
    best = 0
    for p in range(1, len(energy)):
        if energy[p] < energy[best]:
            best = p
    return best


def trial_population(pop, energy, lo, hi, F, seed, gen):
    P, D = pop.shape
    best = best_index(energy)
    trial = pop.copy()
    for i in range(P):
        r0, r1 = select(seed, gen, i, P)
        fill = int(u01(seed, gen, i, 2) * D)
        for a in range(D):
            if a == fill or u01(seed, gen, i, 8 + a) < CR:
                v = float(pop[best, a]) + F * (float(pop[r0, a]) - float(pop[r1, a]))
                if v < lo[a] or v > hi[a]:
                    v = float(lo[a]) + u01(seed, gen, i, 64 + a) * (float(hi[a]) - float(lo[a]))
                trial[i, a] = v
    return trial


def converged(energy, tol, atol):
    """The device host loop's test: all finite and std(energies) <= atol + tol |mean|, sums in index order."""
    P = len(energy)
    mean, var, finite = 0.0, 0.0, True
    for e in energy:
        mean += float(e)
        finite = finite and math.isfinite(e)
    mean /= P
    for e in energy:
        var += (float(e) - mean) * (float(e) - mean)
    return finite and math.sqrt(var / P) <= atol + tol * abs(mean)


def fit_de(energy_fn, bounds, init_pop, seed, maxiter, tol, atol=0.0):
    """Returns (best_x, best_energy, generations) as sbo_fit_de does."""
    bounds = np.asarray(bounds, dtype=np.float64)
    lo, hi = bounds[:, 0], bounds[:, 1]
    pop = np.array(init_pop, dtype=np.float64)
    energy = np.asarray(energy_fn(pop), dtype=np.float64)
    Fs = f_sequence(seed, maxiter)
    gen = 0
    while gen < maxiter:
        trial = trial_population(pop, energy, lo, hi, Fs[gen], seed, gen)
        e = np.asarray(energy_fn(trial), dtype=np.float64)
        take = e <= energy
        pop = np.where(take[:, None], trial, pop)
        energy = np.where(take, e, energy)
        if (gen & 7) == 7 or gen + 1 == maxiter:
            if converged(energy, tol, atol):
                gen += 1
                break
        gen += 1
    best = best_index(energy)
    return pop[best].copy(), float(energy[best]), gen
