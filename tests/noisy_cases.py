"""Cases, float64 references and fp32 restatements for the noisy layers (dq_noisy_draw /
k_noisy_draw, dq_noisy_weights and dq_noisy_grads / k_noisy_apply) -- TEST INFRASTRUCTURE ONLY,
nothing here touches the GPU.

A dense layer of p inputs and q outputs (Fortunato et al. 2018, section 3 (b), eq. 10-11):
  e[j, k] = f_out[j] * f_in[k]            f(n) = sgn(n) sqrt(|n|) of standard normals n
  w[j, k] = mu_w[j, k] + sigma_w[j, k] * e[j, k]        b[j] = mu_b[j] + sigma_b[j] * f_out[j]
  d mu_w = dw    d sigma_w = dw * e    d mu_b = db    d sigma_b = db * f_out
A network's noise buffer is layer-major, [f_in_0 (D) | f_out_0 | f_in_1 | f_out_1 | ...], and
element i of it is draw i of one generator call.

The generator: draw i of call c of generator ``seed`` is z = the splitmix64 hash dq_uniform_draw
uses on (seed, c, i + 1); u1 = ((z >> 40) + 1) * 2^-24 in (0, 1], u2 = ((z >> 16) & 0xFFFFFF) *
2^-24; n = sqrt(-2 ln u1) * cos(2 pi u2).  ``hash_of`` is that hash in Python integers,
``normal64`` the float64 normals.

The float64 references carry the sum of the absolute values of the terms each element adds
(oracle.nature_cnn.cond_ratio's denominator): |mu| + |sigma e| for w and b, |dw e| for d sigma.
The fp32 restatements follow the kernels' order -- e one rounded product f_out * f_in, then
mu + (sigma * e), a rounded product and a rounded sum -- as explicit loops over the rows, so
they must equal the kernels bit for bit.  The ``wrong=`` variants are the mistakes a noisy
layer invites; the tests show that the bar rejects each.
"""
import math

import numpy as np

MASK = (1 << 64) - 1
# the agents' generators: DQNAgent.NOISE_SEED + 256 * the agent's seed (0) + the role's index
ROLE_SEEDS = {'online': 0x4E015E00, 'target': 0x4E015E01, 'act': 0x4E015E02}

# (D, sizes, n_out): what each exercises is in tests/test_gpu_noisy.py's docstring
GEOMETRIES = [(1, (1,), 1), (4, (3,), 2), (6, (5, 7), 3), (4, (64, 64), 102),
              (16, (33, 65, 31, 1), 1024), (6, (1024,), 1024), (4, (512, 512), 153)]


def geometry_id(g):
  return 'D%d-%s-n%d' % (g[0], 'x'.join(str(w) for w in g[1]), g[2])


# ------------------------------------------------------------------ the generator
def hash_of(seed, call, i):
  """The 64-bit hash of draw i of call ``call`` of generator ``seed``, in Python integers."""
  z = (seed + call * 0x9E3779B97F4A7C15 + (i + 1) * 0xD1B54A32D192ED03) & MASK
  z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
  z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
  return z ^ (z >> 31)


def normal64(seed, call, n):
  """The n standard normals of call ``call`` of generator ``seed``, float64."""
  z = [hash_of(seed, call, i) for i in range(n)]
  u1 = (np.array([v >> 40 for v in z], np.float64) + 1.0) * 2.0 ** -24
  u2 = np.array([(v >> 16) & 0xFFFFFF for v in z], np.float64) * 2.0 ** -24
  return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def f64(n, wrong=None):
  """f(n) = sgn(n) sqrt(|n|), float64."""
  n = np.asarray(n, np.float64)
  if wrong == 'f_without_sqrt':
    return n.copy()
  return np.sign(n) * np.sqrt(np.abs(n))


# ------------------------------------------------------------------ layouts
def layers(geometry):
  """[(p, q, offset of f_in, offset of f_out)] per layer of (D, sizes, n_out)."""
  D, sizes, n_out = geometry
  dims = [D] + list(sizes) + [n_out]
  out, off = [], 0
  for l in range(len(dims) - 1):
    p, q = dims[l], dims[l + 1]
    out.append((p, q, off, off + p))
    off += p + q
  return out


def noise_numel(geometry):
  return sum(p + q for p, q, _, _ in layers(geometry))


def sigma_init(geometry, sigma0=0.5, wrong=None):
  """Per layer (sigma_w (q, p), sigma_b (q)) float32 at sigma0 / sqrt(p)."""
  out = []
  for p, q, _, _ in layers(geometry):
    v = np.float32(sigma0 / math.sqrt(q if wrong == 'sigma_over_sqrt_q' else p))
    out.append((np.full((q, p), v, np.float32), np.full(q, v, np.float32)))
  return out


def make_case(geometry, seed, sigma_scale=1.0):
  """mu ~ U(-1 / sqrt(p), 1 / sqrt(p)), sigma = sigma_scale * 0.5 / sqrt(p), dense dw / db, and
  the noise of call 1 of generator ``seed``: float32, fixed seed."""
  rs = np.random.RandomState(seed)
  mu, dw = [], []
  for p, q, _, _ in layers(geometry):
    lim = 1.0 / math.sqrt(p)
    mu.append((rs.uniform(-lim, lim, (q, p)).astype(np.float32),
               rs.uniform(-lim, lim, q).astype(np.float32)))
    dw.append((rs.standard_normal((q, p)).astype(np.float32),
               rs.standard_normal(q).astype(np.float32)))
  sigma = [(w * np.float32(sigma_scale), b * np.float32(sigma_scale))
           for w, b in sigma_init(geometry)]
  normals = normal64(seed, 1, noise_numel(geometry))
  return dict(geometry=geometry, mu=mu, sigma=sigma, dw=dw, normals=normals,
              noise=f64(normals).astype(np.float32))


def _vectors(noise, p, q, fin, fout, wrong):
  """(f_in (p), f_out (q)) of a layer from the noise buffer."""
  f_in, f_out = noise[fin:fin + p], noise[fout:fout + q]
  if wrong == 'one_noise_vector':       # one vector serves both roles
    v = noise[fin:fin + p + q]
    f_in, f_out = v[:p], v[:q]
  return f_in, f_out


# ------------------------------------------------------------------ float64 references
def weights64(geometry, mu, sigma, noise):
  """Per layer (w, b, their Σ|terms|: tw, tb), float64, from the noise buffer given."""
  noise = np.asarray(noise, np.float64)
  out = []
  for (p, q, fin, fout), (mw, mb), (sw, sb) in zip(layers(geometry), mu, sigma):
    f_in, f_out = noise[fin:fin + p], noise[fout:fout + q]
    e = f_out[:, None] * f_in[None, :]
    mw, mb, sw, sb = (np.asarray(a, np.float64) for a in (mw, mb, sw, sb))
    out.append((mw + sw * e, mb + sb * f_out, np.abs(mw) + np.abs(sw * e),
                np.abs(mb) + np.abs(sb * f_out)))
  return out


def grads64(geometry, dw, noise):
  """Per layer (d sigma_w, d sigma_b, their Σ|terms|), float64; d mu is dw / db itself."""
  noise = np.asarray(noise, np.float64)
  out = []
  for (p, q, fin, fout), (gw, gb) in zip(layers(geometry), dw):
    f_in, f_out = noise[fin:fin + p], noise[fout:fout + q]
    e = f_out[:, None] * f_in[None, :]
    gw, gb = np.asarray(gw, np.float64).reshape(q, p), np.asarray(gb, np.float64).reshape(q)
    out.append((gw * e, gb * f_out, np.abs(gw * e), np.abs(gb * f_out)))
  return out


# ------------------------------------------------------------------ fp32 restatements
WEIGHTS_WRONG = ('f_without_sqrt', 'roles_swapped', 'bias_noise_from_f_in', 'sigma_over_sqrt_q',
                 'one_noise_vector')
GRADS_WRONG = ('f_without_sqrt', 'roles_swapped', 'dsigma_without_f_out', 'dmu_times_e',
               'one_noise_vector')


def _e32(f_in, f_out, j, p, q, wrong):
  """Row j of e (p values), float32: f_out[j] * f_in[k], one rounded product."""
  if wrong == 'roles_swapped':          # e[j, k] = f_in[j] * f_out[k]
    return (f_in[j % p] * f_out[np.arange(p) % q]).astype(np.float32)
  return (f_out[j] * f_in).astype(np.float32)


def weights32(geometry, mu, sigma, noise, wrong=None):
  """Per layer (w (q, p), b (q)) float32 in the kernel's order, row by row."""
  noise = np.asarray(noise, np.float32)
  out = []
  for (p, q, fin, fout), (mw, mb), (sw, sb) in zip(layers(geometry), mu, sigma):
    f_in, f_out = _vectors(noise, p, q, fin, fout, wrong)
    w = np.empty((q, p), np.float32)
    for j in range(q):
      e = _e32(f_in, f_out, j, p, q, wrong)
      w[j] = (mw[j] + (sw[j] * e).astype(np.float32)).astype(np.float32)
    fb = f_in[np.arange(q) % p] if wrong == 'bias_noise_from_f_in' else f_out
    b = (mb + (sb * fb).astype(np.float32)).astype(np.float32)
    out.append((w, b))
  return out


def grads32(geometry, dw, noise, wrong=None):
  """Per layer (d mu_w, d mu_b, d sigma_w, d sigma_b) float32 in the kernel's order."""
  noise = np.asarray(noise, np.float32)
  out = []
  for (p, q, fin, fout), (gw, gb) in zip(layers(geometry), dw):
    f_in, f_out = _vectors(noise, p, q, fin, fout, wrong)
    gs = np.empty((q, p), np.float32)
    gm = np.array(gw, np.float32)
    for j in range(q):
      e = _e32(f_in, f_out, j, p, q, wrong)
      if wrong == 'dsigma_without_f_out':
        e = f_in.astype(np.float32)
      gs[j] = (gw[j] * e).astype(np.float32)
      if wrong == 'dmu_times_e':
        gm[j] = gs[j]
    out.append((gm, np.array(gb, np.float32), gs, (gb * f_out).astype(np.float32)))
  return out


# ------------------------------------------------------------------ the float64 network
def rescale32(x, lo, hi):
  """The float32 rescaled input 2 (x - min) / range - 1 (gym_lib.py:95-99)."""
  x = np.asarray(x, np.float64).reshape(len(x), -1).astype(np.float32)
  lo = np.asarray(lo, np.float64)
  rng = (np.asarray(hi, np.float64) - lo).astype(np.float32)
  return np.float32(2.0) * ((x - lo.astype(np.float32)) / rng) - np.float32(1.0)


def mlp64(x0, eff):
  """(the last layer's output, the layers' inputs) of the ReLU MLP on per-layer (w, b, ...)."""
  h, ins = np.asarray(x0, np.float64), []
  for l, layer in enumerate(eff):
    ins.append(h)
    z = h @ layer[0].T + layer[1]
    h = z if l == len(eff) - 1 else np.maximum(z, 0.0)
  return h, ins


def mlp64_backward(eff, ins, gout):
  """Per layer (dw, db) float64 from d loss / d (the last layer's output)."""
  dz, out = np.asarray(gout, np.float64), []
  for layer, x_in in reversed(list(zip(eff, ins))):
    out.append((dz.T @ x_in, dz.sum(0)))
    dz = (dz @ layer[0]) * (x_in > 0)      # the previous layer's ReLU (unused below layer 0)
  return out[::-1]
