"""The host twin of the device differential evolution (tests/de_twin.py) on its own: the draws it restates are well formed."""
import numpy as np

import de_twin


def test_mix64_is_splitmix64():
    # splitmix64's first outputs from state 0 (the generator adds the golden gamma before finalising)
    assert de_twin.mix64(0) == 0xE220A8397B1DCDAF
    assert de_twin.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_selected_members_are_distinct_from_each_other_and_the_candidate():
    for P in (4, 5, 20, 33):
        for seed in (0, 1, 2 ** 64 - 1):
            for gen in range(6):
                for i in range(P):
                    r0, r1 = de_twin.select(seed, gen, i, P)
                    assert len({r0, r1, i}) == 3 and 0 <= r0 < P and 0 <= r1 < P, (P, seed, gen, i, r0, r1)


def test_draws_are_uniform():
    """Chi-square of r0, r1 (over the members other than i) and of the forced crossover entry over many (generation, member)."""
    P, D, i = 9, 6, 4
    c0, c1, cf = np.zeros(P), np.zeros(P), np.zeros(D)
    N = 20000
    for gen in range(N):
        r0, r1 = de_twin.select(12345, gen, i, P)
        c0[r0] += 1
        c1[r1] += 1
        cf[int(de_twin.u01(12345, gen, i, 2) * D)] += 1
    assert c0[i] == 0 and c1[i] == 0
    for c, k in ((np.delete(c0, i), P - 1), (np.delete(c1, i), P - 1), (cf, D)):
        e = N / k
        chi2 = float(np.sum((c - e) ** 2 / e))
        assert chi2 < 3.0 * k + 20, (chi2, c)       # (mean k - 1, sd sqrt(2 (k - 1)))
    u = np.array([de_twin.u01(7, g, 3, 8) for g in range(N)])
    assert abs(u.mean() - 0.5) < 0.01 and np.all((u >= 0) & (u < 1))
    assert abs(np.mean(u < de_twin.CR) - de_twin.CR) < 0.015


def test_f_sequence_is_dithered_in_half_to_one():
    F = de_twin.f_sequence(99, 2000)
    assert min(F) >= 0.5 and max(F) < 1.0 and abs(np.mean(F) - 0.75) < 0.01 and len(set(F)) == 2000


def test_twin_on_a_host_objective():
    """With a NumPy objective the twin is an ordinary DE: bounded, monotone best energy, stops on the tolerance."""
    rng = np.random.default_rng(0)
    B = np.array([[-2.0, 2.0]] * 4)
    pop = rng.uniform(B[:, 0], B[:, 1], size=(16, 4))

    def sphere(p):
        return np.sum((p - 0.3) ** 2, axis=1)

    x, e, g = de_twin.fit_de(sphere, B, pop, seed=3, maxiter=200, tol=1e-3)
    assert e <= float(np.min(sphere(pop))) and np.all(x >= B[:, 0]) and np.all(x <= B[:, 1])
    assert g % 8 == 0 or g == 200
    x0, e0, g0 = de_twin.fit_de(sphere, B, pop, seed=3, maxiter=0, tol=0.0)
    assert g0 == 0 and e0 == float(np.min(sphere(pop)))
