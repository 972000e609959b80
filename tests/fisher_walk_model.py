"""csrc/fisher.hip restated in pure Python float64 (helper module, no tests in here): Walk (side, start, turn, step,
rescale, tail_negligible, TRIP = 8), fisher_two_sided and the pmf(a) evaluations, step for step.

It is NEVER the source of an expected value -- those come from tests/fisher_referee.py.  It has two uses:

- the step budget: how many walk steps the kernel issues for a table is known before the table goes to a GPU
  (tests/test_fisher_referee_cpu.py asserts the limits of tests/test_gpu_pair_large_counts.py's fixtures);
- separating the two factors of p = pmf(a) * (1 + sum): the CPU tests hold the ratio sum alone against the referee.

    fisher(a, b, c, d, unroll=8, table_max=1 << 20) -> Result(p, pmf, total, steps)

unroll = 8 is fisher_two_sided (the tables kernel: Walk.run); 4 .. 24 is a lane of the pair kernel, which issues `unroll`
steps between two end tests and rescales in between when its products have left the first half of the exponent range
(the kernel asks the whole wave; scaling is by exact powers of two, so a lane's sums do not depend on the answer).
Python has no fused multiply-add before 3.13: without math.fma the step's S = fma(S, D, term) rounds twice and the model
is within an ulp per step of the kernel instead of bit for bit.
"""
import math
from collections import namedtuple

Result = namedtuple("Result", "p pmf total steps")

SLACK = 1.0 + 1e-12
INV_SLACK = 1.0 / (1.0 + 1e-12)
TRIP = 8
TABLE_MAX = 1 << 20
MAX_ISSUED = 8_000_000     # the model gives up here (a test table walks 2e6 steps at the most)

_fma = getattr(math, "fma", None) or (lambda x, y, z: x * y + z)


class Walk:
    __slots__ = ("N", "dN", "D", "dD", "P", "Q", "S", "dN_end", "eP", "issued")

    def __init__(self):
        self.issued = 0

    def side(self, u1, u2, v1, v2, steps):
        self.N = u1 * u2
        self.dN = 1.0 - (u1 + u2)
        self.D = v1 * v2
        self.dD = v1 + v2 + 1.0
        self.dN_end = self.dN + 2.0 * steps

    def start(self, u1, u2, v1, v2, steps):
        self.side(u1, u2, v1, v2, steps)
        self.P, self.Q, self.S, self.eP = INV_SLACK, 1.0, 0.0, 0

    def turn(self, u1, u2, v1, v2, steps):
        self.side(u1, u2, v1, v2, steps)
        self.P, self.eP = self.Q * INV_SLACK, 0

    def step(self, ok):
        self.P *= self.N
        self.Q *= self.D
        self.S = _fma(self.S, self.D, self.P if (ok and self.P <= self.Q) else 0.0)
        self.N += self.dN
        self.dN += 2.0
        self.D += self.dD
        self.dD += 2.0
        self.issued += 1

    def at_end(self):
        return self.dN >= self.dN_end

    def tail_negligible(self):
        return self.eP == 0 and self.P <= self.Q and self.N + self.N < self.D and self.P < 1e-13 * (self.Q + self.S)

    def rescale_due(self):
        return self.Q > 2.0 ** 490 or self.P > 2.0 ** 490 or self.eP != 0

    def rescale(self):
        sc = math.ldexp(1.0, 1 - math.frexp(self.Q)[1])          # Q >= 1, a normal number: back into [1, 2)
        self.Q *= sc
        self.S *= sc
        self.P *= sc
        up = self.P > 2.0 ** 500
        dn = self.eP > 0 and self.P < 2.0 ** -3
        if up or dn:
            self.P = math.ldexp(self.P, -500 if up else 500)
            self.eP += 1 if up else -1

    def sum(self):
        # (the kernel: a reciprocal seed and one Newton step, ~1e-14)
        return (self.S * SLACK) / self.Q

    def run(self, unroll=TRIP):
        while True:
            if self.issued > MAX_ISSUED:
                raise OverflowError("fisher_walk_model: more than %d steps: not a table for a test" % MAX_ISSUED)
            ok = self.eP == 0
            for k in range(unroll):
                self.step(ok)
                if k % TRIP == TRIP - 1 and k + 1 < unroll and self.rescale_due():
                    self.rescale()
                    ok = self.eP == 0
            self.rescale()
            if self.at_end() or self.tail_negligible():
                break


# ------------------------------------------------------------------------------ pmf(a)
def log_pmf_table(a, b, c, d):
    """the nine log-factorials (in the table: lgamma(k + 1) of the device; here the host's)"""
    lf = lambda k: math.lgamma(k + 1.0)                                                        # noqa: E731
    return lf(a + b) + lf(c + d) + lf(a + c) + lf(b + d) - lf(a + b + c + d) - lf(a) - lf(b) - lf(c) - lf(d)


def stirling_rest(x):
    """h(x) = log x! - (x log x - x): 0 at 0, lgamma below 16, 0.5 log(2 pi x) + the Stirling series from there on"""
    if x == 0.0:
        return 0.0
    if x < 16.0:
        return math.lgamma(x + 1.0) - (x * math.log(x) - x)
    r = 1.0 / (x * x)
    s = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) * r) * r) * r) * r) / x
    return 0.5 * math.log(6.283185307179586 * x) + s


def deviance_term(x, e, delta):
    """x log(x / e) + e - x for a cell x with expectation e > 0 and delta = x - e given to full precision"""
    if x == 0.0:
        return -delta
    if abs(delta) < 0.1 * (x + e):
        v = delta / (x + e)
        w = v * v
        s = 0.0
        for j in (23.0, 21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0):
            s = (s + 1.0 / j) * w
        s = (s + 1.0 / 3.0) * w
        return delta * v + 2.0 * x * v * s
    return x * math.log(x / e) - delta


def log_pmf_saddle(a, b, c, d):
    """log pmf(a) = h(margins) - h(total) - h(cells) - sum of the cells' deviance terms; every cell is off its expectation
    by the same +-delta = (ad - bc) / total, taken from the exact products"""
    n1, n2, nn, mm = a + b, c + d, a + c, b + d
    M = n1 + n2
    p, q = a * d, b * c
    det = (p - q) + (_fma(a, d, -p) - _fma(b, c, -q))
    delta = det / M
    dev = (deviance_term(a, n1 * nn / M, delta) + deviance_term(b, n1 * mm / M, -delta)
           + deviance_term(c, n2 * nn / M, -delta) + deviance_term(d, n2 * mm / M, delta))
    rest = (stirling_rest(n1) + stirling_rest(n2) + stirling_rest(nn) + stirling_rest(mm)) - stirling_rest(M) - \
        (stirling_rest(a) + stirling_rest(b) + stirling_rest(c) + stirling_rest(d))
    return rest - dev


# ------------------------------------------------------------------------------ fisher_two_sided
def fisher(a, b, c, d, unroll=TRIP, table_max=TABLE_MAX, log_pmf=None):
    """Result(p, pmf = exp(log pmf(a)), total = 1 + sum of the accepted ratios, steps issued); log_pmf overrides the
    kernel's choice (the table below table_max, the saddle-point form from there on)"""
    a, b, c, d = int(a), int(b), int(c), int(d)
    n1, n2, n, m = a + b, c + d, a + c, b + d
    if n1 == 0 or n2 == 0 or n == 0 or m == 0:
        return Result(1.0, 1.0, 1.0, 0)
    fa, fb, fc, fd = float(a), float(b), float(c), float(d)
    if log_pmf is None:
        log_pmf = log_pmf_table if n1 + n2 < table_max else log_pmf_saddle
    pmf = math.exp(log_pmf(fa, fb, fc, fd))
    w = Walk()
    down, up = float(min(a, d)), float(min(b, c))
    w.start(fa, fd, fb + 1.0, fc + 1.0, down)
    if down > 0:
        w.run(unroll)
    w.turn(fb, fc, fa + 1.0, fd + 1.0, up)
    if up > 0:
        w.run(unroll)
    total = 1.0 + w.sum()
    return Result(min(pmf * total, 1.0), pmf, total, w.issued)


def steps(a, b, c, d, unroll=24):
    """walk steps a lane of the pair kernel issues for the table at the longest trip (the most it can overshoot)"""
    return fisher(a, b, c, d, unroll=unroll, log_pmf=lambda *t: 0.0).steps
