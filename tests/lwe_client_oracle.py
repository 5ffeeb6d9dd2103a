"""Pure-Python restatement of the batched client side (TEST INFRASTRUCTURE; the checker of csrc/lwe_client.hip): decoding of LWE phases,
the exact noise statistics, and the test vector of a lookup table.  Python integers only -- the definitions of include/vpbs_prover.h
("the client side in batches") written down a second time, with nothing shared with the product."""
P = 0xFFFFFFFF00000001


def phase(s, ct):
    """what vpbs_lwe_decrypt returns: every word of the row and of the key is reduced below p first"""
    s, ct = [int(v) % P for v in s], [int(v) % P for v in ct]
    assert len(ct) == len(s) + 1
    return (ct[-1] - sum(a * b for a, b in zip(s, ct[:-1]))) % P


def decode(ph, delta, modulus, expected=None):
    """-> (msg, err, failed); err centred into (-p/2, p/2]"""
    msg = ((ph + delta // 2) // delta) % modulus
    ref = msg if expected is None else int(expected)
    err = (ph - ref * delta) % P
    if err > P // 2:
        err -= P
    return msg, err, expected is not None and msg != int(expected) % modulus


class Stats:
    def __init__(self):
        self.count = self.failures = self.max_abs = self.sum_abs = self.sum_sq = self.sum_signed = 0
        self.hist = [0] * 65

    def add(self, err, failed):
        self.count += 1
        self.failures += int(failed)
        self.max_abs = max(self.max_abs, abs(err))
        self.sum_abs += abs(err)
        self.sum_sq += err * err
        self.sum_signed += err
        self.hist[abs(err).bit_length()] += 1

    def as_dict(self):
        return {"count": self.count, "failures": self.failures, "max_abs": self.max_abs, "sum_abs": self.sum_abs, "sum_sq": self.sum_sq,
                "sum_signed": self.sum_signed, "hist": list(self.hist)}


def decode_batch(s, cts, delta, modulus, expected=None, stats=None):
    """-> (phases, msgs, errs) as lists of Python integers; stats (a Stats) is added to"""
    phases, msgs, errs = [], [], []
    for i, ct in enumerate(cts):
        ph = phase(s, ct)
        msg, err, failed = decode(ph, delta, modulus, None if expected is None else expected[i])
        phases.append(ph)
        msgs.append(msg)
        errs.append(err)
        if stats is not None:
            stats.add(err, failed)
    return phases, msgs, errs


def lut_testv(n, p, table, delta):
    """blocks of n / p coefficients table[i] * delta, then Poly::left_shift(block / 2): c[i] <- c[i + s], wrapped terms negated"""
    block = n // p
    coeffs = [int(table[i]) * delta % P for i in range(p) for _ in range(block)]
    s = block // 2
    return [coeffs[i + s] if i + s < n else (P - coeffs[i + s - n]) % P for i in range(n)]


def edge_phases(delta, modulus):
    """the exact half-way points of the rounding, one below and one above, for k = 0 and k = modulus - 1 (the wrap to 0), and err = +-1,
    +-floor(delta / 2) around a message; all below p for delta * modulus <= p"""
    out = []
    for k in (0, modulus - 1):
        h = k * delta + delta // 2
        out += [h - 1, h, h + 1]
    m = 1 % modulus
    out += [(m * delta + e) % P for e in (1, -1, delta // 2, -(delta // 2))]
    return [v % P for v in out]
