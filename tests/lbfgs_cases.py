"""The case table of the L-BFGS kernels (csrc/dpn_lbfgs.inc): tensor lists, history sizes, push sequences and the vectors they are run on.  Imports
without a GPU: tests/test_lbfgs_cpu.py walks the table through the numpy restatements, tests/test_gpu_lbfgs.py through the kernels."""
import collections

import numpy as np

CHUNK = 2048
TensorList = collections.namedtuple('TensorList', 'name numels misaligned')
# numels drawn from 1, 3, 2047, 2048, 2049, 4100: a single element, a tail shorter than a float4, one short of a chunk, a whole chunk, one over, two
# chunks and a tail.  `misaligned`: the index of the tensor whose pointer sits one float off a 16-byte boundary
TENSOR_LISTS = (
    TensorList('small', (3, 2049, 1, 2047), 1),
    TensorList('chunks', (2048, 4100, 3, 2049), 2),
    TensorList('one', (1,), None),
    TensorList('many', (1,) * 161, 7),                  # 161 tensors: two table launches (kAdamFlatMaxTensors = 160)
)
TENSOR_LIST_IDS = tuple(t.name for t in TENSOR_LISTS)
HISTORY_SIZES = (1, 3)
MAGNITUDES = (1e-6, 1e-3, 1.0, 1e3, 1e6)


def tensor_list(name):
    return next(t for t in TENSOR_LISTS if t.name == name)


def push_counts(m):
    """Pairs pushed: none, one, a full ring, past the wrap, twice round and one."""
    return (0, 1, m, m + 2, 2 * m + 1)


def total_floats(numels):
    return sum(-(-n // CHUNK) * CHUNK for n in numels)


def vectors(numels, seed, count):
    """`count` lists of fp32 tensors (one per numel), magnitudes mixed from 1e-6 to 1e+6 element by element."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        out.append([(rng.standard_normal(n) * rng.choice(MAGNITUDES, n)).astype(np.float32) for n in numels])
    return out


Push = collections.namedtuple('Push', 'd g t bad')


def push_sequence(numels, m, pairs, seed, bad_at=None):
    """The inputs of `pairs` pushes: per push a direction d, a step length t and the gradient g AFTER the step, built so that s.y > 1e-10 (g moves
    along d) except for push `bad_at`, whose gradient moves against d (s.y < 0: the pair is refused).  Element 0 of the returned list is the
    start: (None, g0, None, False)."""
    rng = np.random.default_rng(seed)
    g = [(rng.standard_normal(n) * rng.choice(MAGNITUDES, n)).astype(np.float32) for n in numels]
    seq = [Push(None, g, None, False)]
    for k in range(pairs):
        d = [(rng.standard_normal(n) * rng.choice(MAGNITUDES, n)).astype(np.float32) for n in numels]
        t = float(np.float32(rng.choice((1.0, 0.37, 2.5e-3, 8.0))))
        bad = k == bad_at
        sign = np.float32(-1.0 if bad else 1.0)
        curv = [rng.uniform(0.5, 2.0, n).astype(np.float32) for n in numels]
        g = [(gi + sign * np.float32(t) * di * ci).astype(np.float32) for gi, di, ci in zip(g, d, curv)]
        seq.append(Push(d, g, t, bad))
    return seq


# every (tensor list, m, pairs) the GPU test runs, and the one sequence with a refused pair in the middle
SEQUENCES = [(tl.name, m, pairs, None) for tl in TENSOR_LISTS[:2] for m in HISTORY_SIZES for pairs in push_counts(m)]
SEQUENCES += [('one', 3, 5, None), ('many', 3, 5, None), ('small', 3, 6, 2), ('small', 3, 7, 4)]      # ('small', 3, 7, 4): refused in a FULL ring
SEQUENCE_IDS = ['%s-m%d-%dpairs%s' % (n, m, p, '' if b is None else '-bad%d' % b) for n, m, p, b in SEQUENCES]
