"""Q-networks of the reference (atari_lib.py:85-199, gym_lib.py:75-317) in
PyTorch-ROCm, with every parameter a view into ONE flat fp32 buffer.

The flat layout is the MI355X-side design choice: the TF1 Adam / RMSProp
update, the online->target sync and the multi-GPU gradient all-reduce are each
a single kernel / copy / RCCL call over the whole model (4.28 M floats for
Rainbow/Asterix) instead of one per variable.

Input convention: states arrive from the gather kernel as float32 NCHW
(B, stack, 84, 84) already divided by 255 (atari_lib.py:96-97 is fused into the
gather).  TF "SAME" padding is reproduced exactly (conv2 needs the asymmetric
(1, 2) pad).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from dopamine_amd import gin_lite


class FlatParams(object):
  """Allocates named parameter views inside one contiguous fp32 buffer (each
  slice 16-byte aligned) plus a matching flat gradient buffer.  tail_align = (name,
  multiple): zero padding at the end so that the range from parameter ``name`` to the end
  is a whole number of ``multiple`` floats (the Nature-CNN nets: the fc bucket splits into
  world equal 16-byte slices for every world size 1..8 -- the data-parallel exchanges'
  shards, data_parallel.shard_bounds; the padding keeps zero gradients, so every optimizer
  leaves it zero)."""

  def __init__(self, shapes, device, tail_align=None):
    self.offsets = {}
    off = 0
    for name, shape in shapes:
      n = int(np.prod(shape))
      self.offsets[name] = (off, tuple(shape))
      off += (n + 3) // 4 * 4
    self.content_numel = off          # the tensors' floats, before the tail padding
    if tail_align is not None:
      name, multiple = tail_align
      off += -(off - self.offsets[name][0]) % multiple
    self.numel = off
    self.flat = torch.zeros(off, dtype=torch.float32, device=device)
    self.grad = torch.zeros(off, dtype=torch.float32, device=device)
    self.params = {}
    for name, (o, shape) in self.offsets.items():
      n = int(np.prod(shape))
      p = torch.nn.Parameter(self._view(self.flat, o, shape))
      p.grad = self._view(self.grad, o, shape)
      self.params[name] = p

    self.grad_views = [self._view(self.grad, o, s) for o, s in self.offsets.values()]

  def segments(self):
    """(offset, numel) of every parameter inside the flat buffer, in order."""
    return [(o, int(np.prod(s))) for o, s in self.offsets.values()]

  def gather_grads(self):
    """Copy autograd's per-parameter gradients into the flat gradient buffer
    (one multi-tensor copy kernel); returns the flat buffer."""
    ps = list(self.params.values())
    if all(p.grad is not None and p.grad.data_ptr() == v.data_ptr()
           for p, v in zip(ps, self.grad_views)):
      return self.grad
    torch._foreach_copy_(self.grad_views, [p.grad for p in ps])
    return self.grad

  @staticmethod
  def _view(buf, o, shape):
    n = int(np.prod(shape))
    if len(shape) == 4:   # conv filters stored (out, kh, kw, in): channels_last for MIOpen NHWC
      out_c, in_c, kh, kw = shape
      return buf[o:o + n].view(out_c, kh, kw, in_c).permute(0, 3, 1, 2)
    return buf[o:o + n].view(shape)

  def __getitem__(self, name):
    return self.params[name]

  def count(self):
    return sum(int(np.prod(s)) for _, s in self.offsets.values())


def _variance_scaling_uniform(shape, fan_in, factor, gen):
  # tf.contrib.slim.variance_scaling_initializer(factor, 'FAN_IN', uniform=True)
  limit = math.sqrt(3.0 * factor / fan_in)
  return (torch.rand(shape, generator=gen) * 2 - 1) * limit


def _xavier_uniform(shape, fan_in, fan_out, gen):
  # slim default initializer: xavier_initializer(uniform=True)
  limit = math.sqrt(6.0 / (fan_in + fan_out))
  return (torch.rand(shape, generator=gen) * 2 - 1) * limit


def dueling_combine(head, num_actions, num_atoms=None):
  """The dueling head (Wang et al. 2016, eq. 9) as a torch expression, so autograd
  differentiates it.  head (B, (A + 1) * N): columns [0, A * N) the advantage stream
  adv[b, a, z] (z fastest), columns [A * N, (A + 1) * N) the value stream val[b, z];
  num_atoms None: N = 1 and a (B, A) result, else (B, A, N).
  out[b, a, z] = (adv[b, a, z] - sum_a adv[b, a, z] / A) + val[b, z]: what dq_dueling_forward
  computes on the HIP executors."""
  A, N = int(num_actions), int(num_atoms or 1)
  B = head.shape[0]
  adv = head[:, :A * N].reshape(B, A, N)
  val = head[:, A * N:].reshape(B, 1, N)
  out = (adv - adv.sum(1, keepdim=True) / A) + val
  return out.reshape(B, A) if num_atoms is None else out


TORSO = [('conv1', (32, None, 8, 8), 4), ('conv2', (64, 32, 4, 4), 2), ('conv3', (64, 64, 3, 3), 1)]


class _Net(object):
  """Base: owns FlatParams; subclasses define shapes() and forward()."""

  tail_align = None
  dueling = False
  noisy = False

  def __init__(self, device, seed, init='rainbow'):
    self.fp = FlatParams(self.shapes(), device, self.tail_align)
    gen = torch.Generator().manual_seed(seed)
    if self.noisy:          # noisy layers have an initialisation of their own
      with torch.no_grad():
        self._init_noisy(gen, device)
      return
    with torch.no_grad():
      for name, (o, shape) in self.fp.offsets.items():
        if name.endswith('_b'):
          continue  # biases: zeros (slim default)
        if len(shape) == 4:
          fan_in, fan_out = shape[1] * shape[2] * shape[3], shape[0] * shape[2] * shape[3]
        else:
          fan_in, fan_out = shape[1], shape[0]

        def draw(shape, fan_out):
          if init == 'rainbow':
            return _variance_scaling_uniform(shape, fan_in, 1.0 / np.sqrt(3.0), gen)
          return _xavier_uniform(shape, fan_in, fan_out, gen)

        if self.dueling and name == self.HEAD + '_w':
          # two dense layers in one matrix (upstream's FullRainbowNetwork): the advantage
          # block, then the value block, each drawn with its own fan_out
          rows = self.head_rows()
          assert sum(rows) == shape[0]
          w = torch.cat([draw((r,) + tuple(shape[1:]), r) for r in rows])
        else:
          w = draw(shape, fan_out)
        self.fp[name].copy_(w.to(device))

  HEAD = 'fc2'        # the last layer's parameter names: HEAD + '_w' / '_b'

  def head_rows(self):
    """dueling: the last layer's rows as (advantage block, value block)."""
    n = getattr(self, 'N', None) or 1
    return (self.A * n, n)

  def _combine(self, head):
    """The network's output from its last layer's: with ``dueling`` the combined
    (B, A[, N]) head (dueling_combine), else the layer's output itself."""
    n = getattr(self, 'N', None)
    if self.dueling:
      return dueling_combine(head, self.A, n)
    return head if n is None else head.view(-1, self.A, n)

  def forward(self, x):
    return self._combine(self.head(x))

  def parameters(self):
    return list(self.fp.params.values())

  def __call__(self, *a, **k):
    return self.forward(*a, **k)


def _torso(fp, x):
  """Nature-CNN torso with TF SAME padding: 84 -> 21 -> 11 -> 11; 7744 features.

  Activations are channels_last (NHWC in memory: MIOpen's NHWC kernels run
  without layout transposes) and the flatten is in (h, w, c) order, i.e. exactly
  TF's slim.flatten of the reference's NHWC tensors (atari_lib.py:101)."""
  x = x.contiguous(memory_format=torch.channels_last)
  x = F.relu(F.conv2d(x, fp['conv1_w'], fp['conv1_b'], stride=4, padding=2))
  x = F.relu(F.conv2d(F.pad(x, (1, 2, 1, 2)), fp['conv2_w'], fp['conv2_b'], stride=2))
  x = F.relu(F.conv2d(x, fp['conv3_w'], fp['conv3_b'], stride=1, padding=1))
  return x.permute(0, 2, 3, 1).flatten(1)


def _torso_shapes(stack):
  return [('conv1_w', (32, stack, 8, 8)), ('conv1_b', (32,)),
          ('conv2_w', (64, 32, 4, 4)), ('conv2_b', (64,)),
          ('conv3_w', (64, 64, 3, 3)), ('conv3_b', (64,))]


# the fc bucket (fc1_w .. the end) in 4 * lcm(1..8) floats: equal 16-byte slices at any world
# size up to 8 (parallel.PeerExchange, ZeRO-1)
FC_BUCKET_ALIGN = ('fc1_w', 4 * 840)


class NatureDQNNetwork(_Net):
  """atari_lib.py:85-105 -> q_values (B, A)."""
  tail_align = FC_BUCKET_ALIGN

  def __init__(self, num_actions, stack_size=4, device='cuda', seed=0, dueling=False):
    self.A, self.S, self.dueling = num_actions, stack_size, bool(dueling)
    super().__init__(device, seed, init='xavier')

  @property
  def n_out(self):
    """fc2's rows: A, or with ``dueling`` A + 1 (the value stream last)."""
    return self.A + int(self.dueling)

  def shapes(self):
    return _torso_shapes(self.S) + [('fc1_w', (512, 7744)), ('fc1_b', (512,)),
                                    ('fc2_w', (self.n_out, 512)), ('fc2_b', (self.n_out,))]

  def head(self, x):
    """fc2's raw output (B, n_out)."""
    h = F.relu(F.linear(_torso(self.fp, x), self.fp['fc1_w'], self.fp['fc1_b']))
    return F.linear(h, self.fp['fc2_w'], self.fp['fc2_b'])


class RainbowNetwork(_Net):
  """atari_lib.py:108-144 -> logits (B, A, N); q/probabilities derived."""
  tail_align = FC_BUCKET_ALIGN

  def __init__(self, num_actions, num_atoms=51, stack_size=4, device='cuda', seed=0,
               dueling=False):
    self.A, self.N, self.S, self.dueling = num_actions, num_atoms, stack_size, bool(dueling)
    super().__init__(device, seed, init='rainbow')

  @property
  def n_out(self):
    """fc2's rows: A * N, or with ``dueling`` (A + 1) * N (the value stream last)."""
    return (self.A + int(self.dueling)) * self.N

  def shapes(self):
    return _torso_shapes(self.S) + [('fc1_w', (512, 7744)), ('fc1_b', (512,)),
                                    ('fc2_w', (self.n_out, 512)), ('fc2_b', (self.n_out,))]

  def head(self, x):
    """fc2's raw output (B, n_out)."""
    h = F.relu(F.linear(_torso(self.fp, x), self.fp['fc1_w'], self.fp['fc1_b']))
    return F.linear(h, self.fp['fc2_w'], self.fp['fc2_b'])


class ImplicitQuantileNetwork(_Net):
  """atari_lib.py:147-199: quantile_values (N*B, A), rows ordered q*B + b."""

  def __init__(self, num_actions, quantile_embedding_dim=64, stack_size=4, device='cuda', seed=0):
    self.A, self.E, self.S = num_actions, quantile_embedding_dim, stack_size
    super().__init__(device, seed, init='rainbow')
    self._i_pi = (torch.arange(1, self.E + 1, dtype=torch.float32, device=device) * math.pi)

  def shapes(self):
    return _torso_shapes(self.S) + [('emb_w', (7744, self.E)), ('emb_b', (7744,)),
                                    ('fc1_w', (512, 7744)), ('fc1_b', (512,)),
                                    ('fc2_w', (self.A, 512)), ('fc2_b', (self.A,))]

  def forward(self, x, num_quantiles, taus=None):
    B = x.shape[0]
    state = _torso(self.fp, x)                                   # (B, 7744)
    tiled = state.repeat(num_quantiles, 1)                       # tf.tile -> row q*B + b
    if taus is None:
      taus = torch.rand(num_quantiles * B, 1, device=x.device)   # tf.random_uniform
    emb = torch.cos(taus * self._i_pi)                           # (N*B, E)
    emb = F.relu(F.linear(emb, self.fp['emb_w'], self.fp['emb_b']))
    h = F.relu(F.linear(tiled * emb, self.fp['fc1_w'], self.fp['fc1_b']))
    return F.linear(h, self.fp['fc2_w'], self.fp['fc2_b']), taus


class BasicDiscreteDomainNetwork(_Net):
  """gym_lib.py:75-110 (_basic_discrete_domain_network): the observation rescaled to
  [-1, 1] by the domain's MIN / MAX, fully connected ReLU layers of ``network_size``, a
  linear layer of num_actions (Q-values) or num_actions * num_atoms (C51 logits) outputs.
  Xavier-uniform weights, zero biases (slim's defaults).  ``forward`` is the PyTorch path
  (``use_hip_mlp=False``); dopamine_amd.mlp.HipMLP runs the same parameters on the HIP
  kernels.  ``noisy``: factorised-Gaussian noisy layers (Fortunato et al. 2018) -- the names
  above hold mu, a sigma pair per layer follows them all (``shapes``), ``head(x, noise)`` runs
  on mu + sigma * noise and the initialisation is the paper's (``_init_noisy``)."""

  MIN = MAX = None      # the domain's observation bounds (float64), set by subclasses
  GIN_NAME = None       # the reference's configurable, whose network_size binding is honoured
  HEAD = 'out'

  def __init__(self, num_actions, num_atoms=None, stack_size=1, device='cuda', seed=0,
               network_size=None, dueling=False, noisy=False, noisy_sigma0=0.5):
    self.dueling = bool(dueling)
    self.noisy, self.noisy_sigma0 = bool(noisy), float(noisy_sigma0)
    if self.noisy and not self.noisy_sigma0 > 0:
      raise ValueError('noisy_sigma0 must be > 0, got %r' % (noisy_sigma0,))
    if network_size is None:    # the gin binding (acrobot_dqn_network.network_size), or 512-512
      bound = gin_lite.query(self.GIN_NAME) if self.GIN_NAME else {}
      network_size = bound.get('network_size', (512, 512))
    self.A, self.N, self.sizes = num_actions, num_atoms, tuple(int(w) for w in network_size)
    self.D = int(len(self.MIN)) * int(stack_size)
    assert stack_size == 1, 'the classic-control domains stack one observation'
    super().__init__(device, seed, init='xavier')
    self._min = torch.tensor(self.MIN, dtype=torch.float32, device=device)
    self._rng = torch.tensor(self.MAX - self.MIN, dtype=torch.float32, device=device)

  @property
  def n_out(self):
    """The last layer's rows: A * N, or with ``dueling`` (A + 1) * N (the value stream last)."""
    return (self.A + int(self.dueling)) * (self.N or 1)

  def layer_names(self):
    return ['fc%d' % i for i in range(len(self.sizes))] + ['out']

  def shapes(self):
    """The layers' weights and biases -- with ``noisy`` the mu parameters -- then, with
    ``noisy``, every layer's sigma_w / sigma_b AFTER all of them: the mu offsets are the plain
    network's, so whatever reads the layers by name (mlp._params_struct) reads mu."""
    dims = [self.D] + list(self.sizes) + [self.n_out]
    s = []
    for i, n in enumerate(self.layer_names()):
      s += [(n + '_w', (dims[i + 1], dims[i])), (n + '_b', (dims[i + 1],))]
    if self.noisy:
      for i, n in enumerate(self.layer_names()):
        s += [(n + '_sigma_w', (dims[i + 1], dims[i])), (n + '_sigma_b', (dims[i + 1],))]
    return s

  @property
  def mu_numel(self):
    """Floats of the flat buffer's mu region (a plain network: the whole buffer)."""
    return self.fp.offsets['fc0_sigma_w'][0] if self.noisy else self.fp.numel

  @property
  def noise_numel(self):
    """Floats of a noise buffer: [f_in_0 (D) | f_out_0 | f_in_1 | f_out_1 | ...], layer-major."""
    return self.D + 2 * sum(self.sizes) + self.n_out

  def _init_noisy(self, gen, device):
    """Fortunato et al. 2018, section 3.2, factorised noise: for a layer of p inputs mu_w and
    mu_b ~ U(-1 / sqrt(p), 1 / sqrt(p)), sigma_w = sigma_b = sigma0 / sqrt(p).  Drawn layer by
    layer, mu_w then mu_b.  A dueling last layer is one noisy layer (both blocks share p)."""
    for n in self.layer_names():
      w = self.fp[n + '_w']
      p = w.shape[1]
      lim = 1.0 / math.sqrt(p)
      for name in (n + '_w', n + '_b'):
        t = self.fp[name]
        t.copy_(((torch.rand(tuple(t.shape), generator=gen) * 2 - 1) * lim).to(device))
      self.fp[n + '_sigma_w'].fill_(self.noisy_sigma0 / math.sqrt(p))
      self.fp[n + '_sigma_b'].fill_(self.noisy_sigma0 / math.sqrt(p))

  def head(self, x, noise=None):
    """The last layer's raw output (B, n_out).  noise: a (noise_numel,) tensor of f-transformed
    normals (the layout above) -- every layer runs on w = mu_w + sigma_w * (f_out f_in^T),
    b = mu_b + sigma_b * f_out, as a torch expression, so autograd yields the sigma gradients
    (what dq_noisy_weights / dq_noisy_grads compute on the HIP executor); None: the mu
    network."""
    h = x.reshape(x.shape[0], -1).float()
    h = 2.0 * ((h - self._min) / self._rng) - 1.0
    names, off = self.layer_names(), 0
    for n in names:
      w, b = self.fp[n + '_w'], self.fp[n + '_b']
      if noise is not None:
        q, p = w.shape
        f_in, f_out = noise[off:off + p], noise[off + p:off + p + q]
        off += p + q
        w = w + self.fp[n + '_sigma_w'] * (f_out[:, None] * f_in[None, :])
        b = b + self.fp[n + '_sigma_b'] * f_out
      h = F.linear(h, w, b)
      if n != 'out':
        h = F.relu(h)
    return h

  def forward(self, x, noise=None):
    return self._combine(self.head(x, noise))


_CARTPOLE_MIN = np.array([-2.4, -5., -math.pi / 12., -math.pi * 2.])
_CARTPOLE_MAX = np.array([2.4, 5., math.pi / 12., math.pi * 2.])
_ACROBOT_MIN = np.array([-1., -1., -1., -1., -5., -5.])
_ACROBOT_MAX = np.array([1., 1., 1., 1., 5., 5.])


class CartpoleDQNNetwork(BasicDiscreteDomainNetwork):
  """gym_lib.py:113-132: rescale to [-1, 1] then FC 512-512-A."""

  MIN, MAX = _CARTPOLE_MIN, _CARTPOLE_MAX
  GIN_NAME = 'cartpole_dqn_network'

  def __init__(self, num_actions, device='cuda', seed=0, network_size=None, num_atoms=None,
               stack_size=1, dueling=False, noisy=False, noisy_sigma0=0.5):
    assert num_atoms is None
    super().__init__(num_actions, None, stack_size, device, seed, network_size, dueling, noisy,
                     noisy_sigma0)


class CartpoleRainbowNetwork(BasicDiscreteDomainNetwork):
  """gym_lib.py:227-252 -> logits (B, A, N)."""

  MIN, MAX = _CARTPOLE_MIN, _CARTPOLE_MAX
  GIN_NAME = 'cartpole_rainbow_network'

  def __init__(self, num_actions, num_atoms=51, stack_size=1, device='cuda', seed=0,
               network_size=None, dueling=False, noisy=False, noisy_sigma0=0.5):
    super().__init__(num_actions, num_atoms, stack_size, device, seed, network_size, dueling,
                     noisy, noisy_sigma0)


class AcrobotDQNNetwork(BasicDiscreteDomainNetwork):
  """gym_lib.py:255-273: rescale to [-1, 1] then FC 512-512-A."""

  MIN, MAX = _ACROBOT_MIN, _ACROBOT_MAX
  GIN_NAME = 'acrobot_dqn_network'

  def __init__(self, num_actions, device='cuda', seed=0, network_size=None, num_atoms=None,
               stack_size=1, dueling=False, noisy=False, noisy_sigma0=0.5):
    assert num_atoms is None
    super().__init__(num_actions, None, stack_size, device, seed, network_size, dueling, noisy,
                     noisy_sigma0)


class AcrobotRainbowNetwork(BasicDiscreteDomainNetwork):
  """gym_lib.py:295-317 -> logits (B, A, N)."""

  MIN, MAX = _ACROBOT_MIN, _ACROBOT_MAX
  GIN_NAME = 'acrobot_rainbow_network'

  def __init__(self, num_actions, num_atoms=51, stack_size=1, device='cuda', seed=0,
               network_size=None, dueling=False, noisy=False, noisy_sigma0=0.5):
    super().__init__(num_actions, num_atoms, stack_size, device, seed, network_size, dueling,
                     noisy, noisy_sigma0)


def fourier_multipliers(in_dim, order):
  """gym_lib.py:153-157: itertools.product(range(order + 1), repeat=in_dim) without its first,
  all-zero tuple, (F, D) int64: row f holds the digits of f + 1 in base order + 1, dimension
  0 the most significant."""
  base, F = order + 1, (order + 1) ** in_dim - 1
  n = np.arange(1, F + 1, dtype=np.int64)[:, None]
  return (n // base ** np.arange(in_dim - 1, -1, -1, dtype=np.int64)[None, :]) % base


class FourierDQNNetwork(_Net):
  """gym_lib.py:135-206 (FourierBasis, fourier_dqn_network): the observation scaled to [0, 1]
  by the domain's MIN / MAX (no clipping), the F = (order + 1)^D - 1 features
  cos(float32(pi) * s . m_f), and a linear layer of num_actions Q-values without a bias
  (Xavier-uniform): the only parameter.  ``forward`` is the PyTorch path
  (``use_hip_mlp=False``); dopamine_amd.fourier.HipFourier runs the same parameter on the HIP
  kernels.  ``fourier_basis_order`` None: the gin binding
  fourier_dqn_network.fourier_basis_order, or 3."""

  MIN = MAX = None      # the domain's observation bounds (float64), set by subclasses
  PI = float(np.float32(np.pi))     # np.pi enters the reference's graph as a float32 constant

  def __init__(self, num_actions, device='cuda', seed=0, fourier_basis_order=None, stack_size=1):
    if fourier_basis_order is None:
      fourier_basis_order = gin_lite.query('fourier_dqn_network').get('fourier_basis_order', 3)
    assert stack_size == 1, 'the classic-control domains stack one observation'
    self.A, self.order = num_actions, int(fourier_basis_order)
    self.D = int(len(self.MIN)) * int(stack_size)
    if self.order < 1:
      raise ValueError('fourier_basis_order must be >= 1, got %r' % (fourier_basis_order,))
    self.F = (self.order + 1) ** self.D - 1
    super().__init__(device, seed, init='xavier')
    self._min = torch.tensor(self.MIN, dtype=torch.float32, device=device)
    self._rng = torch.tensor(self.MAX - self.MIN, dtype=torch.float32, device=device)
    self._mult = torch.tensor(fourier_multipliers(self.D, self.order), dtype=torch.float32,
                              device=device)

  @property
  def n_out(self):
    return self.A

  def shapes(self):
    return [('out_w', (self.A, self.F))]

  def features(self, x):
    """(the scaled input (B, D), the features (B, F)), float32."""
    s = (x.reshape(x.shape[0], -1).float() - self._min) / self._rng
    return s, torch.cos(self.PI * (s @ self._mult.t()))

  def forward(self, x):
    return F.linear(self.features(x)[1], self.fp['out_w'])


class CartpoleFourierDQNNetwork(FourierDQNNetwork):
  """gym_lib.py:209-224: 255 features at order 3, 510 parameters."""

  MIN, MAX = _CARTPOLE_MIN, _CARTPOLE_MAX


class AcrobotFourierDQNNetwork(FourierDQNNetwork):
  """gym_lib.py:276-292: 4,095 features at order 3, 12,285 parameters."""

  MIN, MAX = _ACROBOT_MIN, _ACROBOT_MAX
