"""Inputs shared by tests/test_c51_wide_reference_cpu.py (which proves, with the oracle alone,
that the measure has margin and power on these inputs and that each input has the property
it was chosen for) and tests/test_gpu_c51_wide.py (which runs dq_c51_loss's wide kernel,
k_c51_wide, on the same inputs).  Built with oracle/learner_cases.py's c51_case; nothing here
touches the GPU.  Cases and their float64 references are built once and shared: treat them
as read-only."""
import functools

import numpy as np

from oracle import learner_cases as C

VMAXES = (10.0, 100.0)

# (B, A, N) of the wide kernel (65 <= N <= 256: a row is 2..4 chunks of 64 atoms, a wave owns
# rows w, w + 4, ..)
SHAPES = (
    (1, 1, 65),      # first atom past a wave, one row, one sample
    (3, 2, 128),     # exactly two chunks
    (5, 3, 129),     # one atom into the third chunk
    (2, 5, 201),     # the reference config's atom count, rows > waves
    (3, 17, 201),    # several rows per wave
    (2, 64, 256),    # both limits at once
    (65, 2, 70),     # B > 64 with PER: the smallest probability at index 64
    (4, 1, 255),     # last lane of the last chunk off
)
MIN_PROB_LAST = (65, 2, 70)
DETERMINISM_SHAPE = (3, 17, 201)


@functools.lru_cache(maxsize=None)
def case(B, A, N, scale, vmax, cg=None, all_terminal=False):
  kw = {} if cg is None else dict(cg=cg)
  c = C.c51_case(B, A, N, scale, vmax=vmax, all_terminal=all_terminal, **kw)
  if vmax == 100.0 and B >= 2:
    c['rew'][0], c['rew'][1] = 300.0, -300.0      # two samples outside the wide support too
  if (B, A, N) == MIN_PROB_LAST:
    c['probs'][64] = 0.01
  return c


def table():
  """(id, case, probs?) of every case the GPU test runs against float64 (the tie case apart)."""
  out = []
  for B, A, N in SHAPES:
    for scale in C.SCALES:
      for vmax in VMAXES:
        c = case(B, A, N, scale, vmax)
        for probs in (True, False):
          out.append(('B%d-A%d-N%d-x%d-v%d-%s' % (B, A, N, scale, vmax, 'per' if probs else 'uni'),
                      c, probs))
  out.append(('gamma0', case(5, 3, 129, 2, 10.0, cg=0.0), True))
  out.append(('all-terminal', case(7, 2, 70, 2, 10.0, all_terminal=True), True))
  return out


_REFS = {}


def reference(name, c, probs):
  """The float64 reference of a table entry, computed once."""
  key = (name, probs)
  if key not in _REFS:
    _REFS[key] = C.c51_reference(c, probs)
  return _REFS[key]


# ---- exact ties of the greedy action on a wide support: 129 atoms on (i - 64) / 4, three
# target rows with logit 0 on atoms k and 128 - k (z_k = -z_{128-k}) and -1000 elsewhere: the
# softmax is exactly 1/2, 1/2 (k = 64: exactly 1) and 0 in fp32 and in float64, every product
# z_i p_i is exact and the non-zero ones cancel, so Q is exactly 0 in any order of the sum.
# k = 3 sits in the first chunk with its mirror in the second, 64 is the first atom of the
# second chunk, 70's mirror 58 is in the first.
TIE_N = 129
TIE_KS = (3, 64, 70)


def tie_case():
  """One sample per order (C.TIE_ORDERS) of the three rows; zero online logits, so
  proj = 1/N - B grad."""
  N, A, B = TIE_N, len(TIE_KS), len(C.TIE_ORDERS)
  z = ((np.arange(N) - 64) / 4.0).astype(np.float32)
  rows = np.full((A, N), -1000.0, np.float32)
  for r, k in enumerate(TIE_KS):
    rows[r, k] = rows[r, N - 1 - k] = 0.0
  tl = np.array([[rows[r] for r in order] for order in C.TIE_ORDERS], np.float32)
  return dict(B=B, A=A, N=N, ol=np.zeros((B, A, N), np.float32), tl=tl,
              act=np.array([0, 1, 2, 0], np.int32),
              rew=np.array([0.25, 0.25, 0.25, -0.25], np.float32),
              term=np.zeros(B, np.uint8), z=z, cg=np.float32(0.5),
              probs=np.array([0.5, 1.0, 0.25, 2.0], np.float32))
