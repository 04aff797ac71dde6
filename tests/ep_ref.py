"""An independent plain-Python statement of mas_episode_stats
(include/masurvival.h), for the tests of its torch restatement and of the
kernel.  Python floats are fp64, so the per-env walk below performs the
kernel's operations in the kernel's order; only the sums across envs have no
prescribed order, and those are held to a bound around math.fsum totals:

  sum_G[a]   n terms G, any order of fp64 adds:      |err| <= n 2^-53 sum|G|
  sum_G2[a]  each product rounded once, then summed: |err| <= (n + 1) 2^-53 sum G^2

(n - 1 roundings of relative 2^-53 on partial sums that never exceed sum|term|,
the half ulp of the fsum total itself, and one rounding per product; the
derivation tests/ret_ref.py uses, plus the product's rounding).  The integer
entries are exact."""
import math

HEAD = ('episodes', 'sum_len', 'sum_len2', 'wins0', 'wins1', 'draws')
U = 2.0 ** -53


def walk(rewards, dones, n_agents, ret_carry, len_carry, side_mask=0):
    """rewards [T][E * A] (fp32 values), dones [T][E] (any nonzero is done),
    the carries going in.  Returns (G [E * A] floats, len [E] ints, counts: a
    dict of the six integer entries as Python ints, ep_G: per agent slot the
    list of the finished episodes' returns in env-major order)."""
    A, T, E = int(n_agents), len(rewards), len(len_carry)
    two = side_mask != 0 and side_mask != (1 << A) - 1
    c = dict.fromkeys(HEAD, 0)
    ep_G = [[] for _ in range(A)]
    G_out, len_out = [], []
    for e in range(E):
        G = [float(ret_carry[e * A + a]) for a in range(A)]
        n = int(len_carry[e])
        for t in range(T):
            row = rewards[t]
            for a in range(A):
                G[a] += float(row[e * A + a])
            n += 1
            if dones[t][e] != 0:
                c['episodes'] += 1
                c['sum_len'] += n
                c['sum_len2'] += n * n
                s0 = s1 = 0.0
                for a in range(A):
                    ep_G[a].append(G[a])
                    if (side_mask >> a) & 1:
                        s0 += G[a]
                    else:
                        s1 += G[a]
                if two:
                    c['wins0'] += s0 > s1
                    c['wins1'] += s1 > s0
                    c['draws'] += s0 == s1
                G = [0.0] * A
                n = 0
        G_out += G
        len_out.append(n)
    return G_out, len_out, c, ep_G


def record(counts, ep_G):
    """The record [episodes, ..., draws, sum_G[A], sum_G2[A]] with fsum totals."""
    return ([float(counts[k]) for k in HEAD] + [math.fsum(g) for g in ep_G]
            + [math.fsum(x * x for x in g) for g in ep_G])


def check_sums(got, counts, ep_G):
    """The worst |got - fsum total| / bound over sum_G and sum_G2 (0 where both
    are 0; inf where the bound is 0 and the entry is not the total)."""
    A, n = len(ep_G), counts['episodes']
    worst = 0.0
    for a in range(A):
        g = ep_G[a]
        for val, ref, bound in ((got[6 + a], math.fsum(g), n * U * math.fsum(abs(x) for x in g)),
                                (got[6 + A + a], math.fsum(x * x for x in g),
                                 (n + 1) * U * math.fsum(x * x for x in g))):
            err = abs(float(val) - ref)
            if err != err:
                worst = math.inf
            elif err > 0.0:
                worst = max(worst, err / bound if bound > 0.0 else math.inf)
    return worst
