"""The networks' ``dueling`` option on the CPU (device='cpu'): shapes, initialisation, the
PyTorch ``forward`` and its autograd against tests/dueling_cases.py's float64 references, and
the non-dueling networks' parameters unchanged draw for draw.  No GPU.
"""
import hashlib
import math

import numpy as np
import pytest
import torch

from dopamine_amd.agents import networks
from tests import dueling_cases as DC

GYM = [(networks.CartpoleRainbowNetwork, 2, 51), (networks.AcrobotRainbowNetwork, 3, 51),
       (networks.CartpoleDQNNetwork, 2, None), (networks.AcrobotDQNNetwork, 3, None)]


def _make(cls, A, N, **kw):
  if N is None:
    return cls(A, device='cpu', **kw)
  return cls(A, num_atoms=N, device='cpu', **kw)


def _state(net, B, seed=3):
  rs = np.random.RandomState(seed)
  if hasattr(net, 'MIN'):
    return torch.from_numpy(rs.uniform(net.MIN, net.MAX, size=(B, len(net.MIN))))
  return torch.from_numpy(rs.rand(B, 4, 84, 84).astype(np.float32))


@pytest.mark.parametrize('cls,A,N', GYM)
def test_gym_network_shapes_and_counts(cls, A, N):
  plain, duel = _make(cls, A, N), _make(cls, A, N, dueling=True)
  n = N or 1
  assert plain.dueling is False and duel.dueling is True
  assert plain.n_out == A * n and duel.n_out == (A + 1) * n
  H = duel.sizes[-1]
  assert duel.fp.offsets['out_w'][1] == ((A + 1) * n, H)
  assert duel.fp.offsets['out_b'][1] == ((A + 1) * n,)
  assert duel.fp.count() - plain.fp.count() == n * (H + 1)      # the value stream's rows
  assert list(duel.fp.offsets) == list(plain.fp.offsets)         # the names kept
  x = _state(duel, 5)
  assert tuple(duel.head(x).shape) == (5, (A + 1) * n)
  assert tuple(duel(x).shape) == ((5, A) if N is None else (5, A, N))
  assert tuple(plain(x).shape) == tuple(duel(x).shape)


@pytest.mark.parametrize('cls,N', [(networks.NatureDQNNetwork, None), (networks.RainbowNetwork, 51)])
def test_nature_network_shapes_and_counts(cls, N):
  A, n = 4, N or 1
  plain, duel = _make(cls, A, N), _make(cls, A, N, dueling=True)
  assert plain.dueling is False and duel.dueling is True
  assert plain.n_out == A * n and duel.n_out == (A + 1) * n
  assert duel.fp.offsets['fc2_w'][1] == ((A + 1) * n, 512)
  assert duel.fp.offsets['fc2_b'][1] == ((A + 1) * n,)
  assert duel.fp.count() - plain.fp.count() == n * 513
  x = _state(duel, 2)
  with torch.no_grad():
    assert tuple(duel.head(x).shape) == (2, (A + 1) * n)
    assert tuple(duel(x).shape) == ((2, A) if N is None else (2, A, N))


def test_fourier_networks_take_no_dueling_argument():
  with pytest.raises(TypeError):
    networks.CartpoleFourierDQNNetwork(2, device='cpu', dueling=True)


NETS = GYM + [(networks.NatureDQNNetwork, 4, None), (networks.RainbowNetwork, 4, 51)]


@pytest.mark.parametrize('cls,A,N', NETS)
def test_forward_is_the_reference_on_the_raw_head_and_autograd_its_backward(cls, A, N):
  net = _make(cls, A, N, dueling=True)
  n = N or 1
  with torch.no_grad():     # non-zero biases, as after training
    for name, prm in net.fp.params.items():
      if name.endswith('_b'):
        prm.uniform_(-0.05, 0.1)
  B = 3
  x = _state(net, B)
  head = net.head(x)
  head.retain_grad()
  out = net._combine(head)
  with torch.no_grad():
    again = net(x)
  assert torch.equal(again, out.detach())
  ref, _ = DC.forward64(head.detach().numpy(), A, n)
  got = out.detach().numpy().reshape(B, A, n)
  assert float(np.abs(got - ref).max()) <= 1e-6 * float(np.abs(ref).max())
  g = np.random.RandomState(4).standard_normal((B, A, n)).astype(np.float32)
  out.backward(torch.from_numpy(g).reshape(out.shape))
  want, _ = DC.backward64(g, A, n)
  assert float(np.abs(head.grad.numpy() - want).max()) <= 1e-6 * float(np.abs(want).max())
  # and it reaches the parameters: the last layer's bias gradient is dhead summed over samples
  bias = net.fp[net.HEAD + '_b'].grad.numpy()
  assert float(np.abs(bias - want.sum(0)).max()) <= 1e-5 * float(np.abs(want.sum(0)).max())


# sha256 of fp.flat at the default seed with a CPU generator, taken on the commit before the
# dueling option existed: with dueling=False not one draw may move
DIGESTS = [
    (networks.CartpoleRainbowNetwork, 2,
     'd2c45a6a3b986bdae2de4c4b20d5c9bc880b4d36312975933a470c4c989bbf60'),
    (networks.AcrobotDQNNetwork, 3,
     '92bf239e8957848af127fb8b1e506369c5df235c8d525f90d36cfd20cb43e7f3'),
    (networks.RainbowNetwork, 4,
     'bd84c327b00854afd9eb0f81212022335d50c7e534bdcc451023143469c277e5'),
    (networks.NatureDQNNetwork, 4,
     'fd3df2bfdaed1ec55a5d5307f5495bb9199c927ea6598b5ab9960f582c5ad807'),
]


@pytest.mark.parametrize('cls,A,digest', DIGESTS)
def test_non_dueling_parameters_are_unchanged(cls, A, digest):
  for kw in ({}, {'dueling': False}):
    net = cls(A, device='cpu', **kw)
    assert hashlib.sha256(net.fp.flat.numpy().tobytes()).hexdigest() == digest


@pytest.mark.parametrize('cls,A,N', [(networks.CartpoleRainbowNetwork, 2, 51),
                                     (networks.AcrobotDQNNetwork, 3, None),
                                     (networks.NatureDQNNetwork, 4, None)])
def test_xavier_blocks_use_their_own_fan_out(cls, A, N):
  """Two dense layers in one matrix: each block uniform within sqrt(6 / (fan_in + its rows)),
  and wide enough to show that limit is its own."""
  net = _make(cls, A, N, dueling=True)
  n = N or 1
  w = net.fp[net.HEAD + '_w'].detach().numpy()
  fan_in = w.shape[1]
  adv, val = w[:A * n], w[A * n:]
  assert val.shape[0] == n
  for block, rows in ((adv, A * n), (val, n)):
    limit = math.sqrt(6.0 / (fan_in + rows))
    assert float(np.abs(block).max()) <= limit
    assert float(np.abs(block).max()) >= 0.9 * limit        # (hundreds of uniform draws)
  # the blocks are consecutive draws of one generator: the advantage block is the plain
  # network's last layer, drawn with the same fan_out at the same point of the stream
  plain = _make(cls, A, N)
  assert np.array_equal(adv, plain.fp[net.HEAD + '_w'].detach().numpy())
  assert not net.fp[net.HEAD + '_b'].detach().numpy().any()


def test_rainbow_initialiser_blocks_coincide_with_one_draw():
  """The 'rainbow' fan-in initialiser ignores fan_out: two blocks from the same generator
  are the one (A + 1) * N-row draw."""
  net = networks.RainbowNetwork(4, num_atoms=5, device='cpu', dueling=True)
  gen = torch.Generator().manual_seed(0)
  for name, (o, shape) in net.fp.offsets.items():
    if name.endswith('_b'):
      continue
    fan_in = int(np.prod(shape[1:]))
    w = networks._variance_scaling_uniform(shape, fan_in, 1.0 / np.sqrt(3.0), gen)
    if name == 'fc2_w':
      assert torch.equal(net.fp['fc2_w'].detach(), w)
