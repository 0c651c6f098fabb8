"""Cases, float64 references and fp32 restatements for the dueling head
(dq_dueling_forward / k_dueling_fwd, dq_dueling_backward / k_dueling_bwd) -- TEST
INFRASTRUCTURE ONLY, nothing here touches the GPU.

head (B, (A + 1) * N): columns [0, A * N) the advantage stream adv[b, a, z] (z fastest),
columns [A * N, (A + 1) * N) the value stream val[b, z].
  out[b, a, z]  = (adv[b, a, z] - sum_a adv[b, a, z] / A) + val[b, z]
  dval[b, z]    = sum_a g[b, a, z]
  dadv[b, a, z] = g[b, a, z] - dval[b, z] / A
The float64 references carry the sum of the absolute values of the terms each element adds
(oracle.nature_cnn.cond_ratio's denominator):
  out    |adv[a]| + mean_a |adv| + |val|
  dval   sum_a |g|
  dadv   |g[a]| + sum_a |g| / A
The fp32 restatements follow the kernels' order -- the sums sequential in action order from
action 0's element, ONE correctly rounded quotient by A, the subtraction before the addition
of val -- as explicit loops over actions, so they must equal the kernels bit for bit.  Their
``wrong=`` variants are the mistakes a dueling head invites; the tests show that the bar
rejects each.
"""
import numpy as np

# (B, A, N): what each exercises is in tests/test_gpu_dueling.py's docstring
SHAPES = [(1, 1, 1), (1, 2, 1), (32, 2, 1), (33, 3, 1), (128, 18, 1), (1, 2, 51), (32, 2, 51),
          (4, 3, 64), (8, 2, 64), (33, 3, 65), (5, 18, 51), (32, 4, 101), (128, 2, 200),
          (3, 3, 255), (7, 64, 256)]
# input kinds: normal at scale 1 / 100; the value stream at 1000 times the advantage's scale
# and the reverse
KINDS = ('n1', 'n100', 'val1000', 'adv1000')
_SCALES = {'n1': (1.0, 1.0), 'n100': (100.0, 100.0), 'val1000': (1.0, 1000.0),
           'adv1000': (1000.0, 1.0)}


def case_id(c):
  return '%dx%dx%d-%s' % (c['B'], c['A'], c['N'], c['kind'])


def make_case(B, A, N, kind, seed):
  """head (B, (A + 1) * N), g (B, A, N) dense, gs (B, A, N) zero off one action per sample (as
  every loss kernel emits) with its taken actions act (B,): float32, fixed seed."""
  rs = np.random.RandomState(seed)
  sa, sv = _SCALES[kind]
  adv = (rs.standard_normal((B, A * N)) * sa).astype(np.float32)
  val = (rs.standard_normal((B, N)) * sv).astype(np.float32)
  head = np.ascontiguousarray(np.concatenate([adv, val], axis=1))
  g = (rs.standard_normal((B, A, N)) * sa).astype(np.float32)
  act = rs.randint(0, A, size=B)
  gs = np.zeros_like(g)
  gs[np.arange(B), act] = g[np.arange(B), act]
  return dict(B=B, A=A, N=N, kind=kind, head=head, g=g, gs=gs, act=act)


def all_cases():
  """Every shape with every input kind, seeds fixed by position."""
  return [make_case(B, A, N, kind, 1000 + 10 * i + j)
          for i, (B, A, N) in enumerate(SHAPES) for j, kind in enumerate(KINDS)]


def split(head, A, N):
  """(adv (B, A, N), val (B, N)) views of head (B, (A + 1) * N)."""
  B = head.shape[0]
  head = head.reshape(B, (A + 1) * N)
  return head[:, :A * N].reshape(B, A, N), head[:, A * N:].reshape(B, N)


# ------------------------------------------------------------------ float64 references
def forward64(head, A, N):
  """(out (B, A, N), its Σ|terms|), float64."""
  adv, val = split(np.asarray(head, np.float64), A, N)
  out = (adv - adv.mean(1, keepdims=True)) + val[:, None, :]
  terms = np.abs(adv) + np.abs(adv).mean(1, keepdims=True) + np.abs(val)[:, None, :]
  return out, terms


def backward64(g, A, N):
  """(dhead (B, (A + 1) * N), its Σ|terms|), float64, from g = d loss / d out (B, A, N)."""
  g = np.asarray(g, np.float64).reshape(-1, A, N)
  B = g.shape[0]
  dval, sabs = g.sum(1), np.abs(g).sum(1)
  dadv = g - dval[:, None, :] / A
  dhead = np.concatenate([dadv.reshape(B, A * N), dval], axis=1)
  terms = np.concatenate([(np.abs(g) + sabs[:, None, :] / A).reshape(B, A * N), sabs], axis=1)
  return dhead, terms


# ------------------------------------------------------------------ fp32 restatements
FORWARD_WRONG = ('divide_by_A_plus_1', 'mean_over_atoms', 'value_at_column_A',
                 'value_before_the_mean')
BACKWARD_WRONG = ('no_mean_term', 'dval_from_the_taken_action', 'blocks_swapped')


def _seq_sum(x):
  """((x[:, 0] + x[:, 1]) + x[:, 2]) + ... over axis 1, float32, one action at a time."""
  s = x[:, 0].copy()
  for a in range(1, x.shape[1]):
    s = (s + x[:, a]).astype(np.float32)
  return s


def forward32(head, A, N, wrong=None):
  """out (B, A, N) float32 in the kernel's order."""
  head = np.asarray(head, np.float32)
  adv, val = split(head, A, N)
  B = adv.shape[0]
  fA = np.float32(A + 1 if wrong == 'divide_by_A_plus_1' else A)
  if wrong == 'value_at_column_A':
    val = head.reshape(B, -1)[:, A:A + N]
  if wrong == 'value_before_the_mean':      # the mean of adv + val takes the value out again
    t = (adv + val[:, None, :]).astype(np.float32)
    m = (_seq_sum(t) / fA).astype(np.float32)
    return (t - m[:, None, :]).astype(np.float32)
  if wrong == 'mean_over_atoms':
    s = adv[:, :, 0].copy()
    for z in range(1, N):
      s = (s + adv[:, :, z]).astype(np.float32)
    m = np.repeat((s / np.float32(N)).astype(np.float32)[:, :, None], N, axis=2)
  else:
    m = (_seq_sum(adv) / fA).astype(np.float32)
  out = np.empty((B, A, N), np.float32)
  for a in range(A):
    ma = m[:, a] if wrong == 'mean_over_atoms' else m
    out[:, a] = ((adv[:, a] - ma).astype(np.float32) + val).astype(np.float32)
  return out


def backward32(g, A, N, wrong=None, act=None):
  """dhead (B, (A + 1) * N) float32 in the kernel's order.  act: the taken actions, for the
  wrong variant that reads only their rows."""
  g = np.asarray(g, np.float32).reshape(-1, A, N)
  B = g.shape[0]
  if wrong == 'dval_from_the_taken_action':
    dval = g[np.arange(B), act].copy()
  else:
    dval = _seq_sum(g)
  q = (dval / np.float32(A)).astype(np.float32)
  if wrong == 'no_mean_term':
    q = np.zeros_like(q)
  dadv = np.empty((B, A, N), np.float32)
  for a in range(A):
    dadv[:, a] = (g[:, a] - q).astype(np.float32)
  blocks = [dadv.reshape(B, A * N), dval]
  if wrong == 'blocks_swapped':
    blocks = blocks[::-1]
  return np.ascontiguousarray(np.concatenate(blocks, axis=1))
