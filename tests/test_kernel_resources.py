"""tools/kernel_resources.py on a recorded remark log (tests/golden/kernel_resource_remarks.log:
one k_igemm block in the compiler's source-echo form; the unpaired 4-class sub-pixel launch
and backward launch 3 with a rider before the sub-pixel tiles took K and N as constants; and
launch 3 with a rider after)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_resources as kr  # noqa: E402

LOG = os.path.join(ROOT, 'tests', 'golden', 'kernel_resource_remarks.log')


def _recs():
  with open(LOG) as f:
    return kr.parse_remarks(f.read())


def test_parses_every_field_of_both_remark_forms():
  recs = _recs()
  assert len(recs) == 4
  assert recs[0]['name'].startswith('_ZN2dq3cnn7k_igemm')
  assert recs[0] == dict(name=recs[0]['name'], sgprs=48, vgprs=63, agprs=0, scratch=0, occupancy=8,
                         sgpr_spill=0, vgpr_spill=0, lds=32768)
  assert [(r['vgprs'], r['vgpr_spill'], r['scratch'], r['sgpr_spill'], r['lds'], r['occupancy'])
          for r in recs[1:]] == [(64, 8, 20, 0, 34816, 8), (64, 49, 76, 182, 73728, 8),
                                 (58, 0, 0, 206, 73728, 8)]


def test_short_names_list_the_ops_in_launch_order():
  dem = ('void dq::cnn::k_grouped<1024, dq::cnn::RiderOpT<false>, dq::cnn::GemmOp<1, 1, 16, '
         'dq::cnn::DyT<64>, dq::cnn::Im2colT<dq::cnn::Conv<11, 11, 64, 3, 3, 1, 1, 1, 11, 11, 64>>, '
         'dq::cnn::EpiPartial, true, 0, 0>, dq::cnn::PairOp<dq::cnn::GemmOp<1, 1, 8, '
         'dq::cnn::SubPixDy<dq::cnn::Conv<21, 21, 32, 4, 4, 2, 1, 1, 11, 11, 64>, 0, 1>, '
         'dq::cnn::SubPixW<dq::cnn::Conv<21, 21, 32, 4, 4, 2, 1, 1, 11, 11, 64>, 0, 1>, '
         'dq::cnn::EpiMaskPix<dq::cnn::SubPix<dq::cnn::Conv<21, 21, 32, 4, 4, 2, 1, 1, 11, 11, 64>, '
         '0, 1>, 32>, true, 256, 32>>>(dq::cnn::GroupArgs<dq::cnn::RiderOpT<false>>, '
         'dq::cnn::RiderOpT<false>)')
  assert kr.short_kernel(dem) == (
      'k_grouped<1024: Rider | Gemm<1,1,16,true,0,0 DyT<64>,Im2colT<>,EpiPartial> | '
      'Pair<Gemm<1,1,8,true,256,32 SubPixDy<0,1>,SubPixW<0,1>,EpiMaskPix<32 SubPix<0,1>>>>>')
  assert kr.short_kernel('void dq::k_mean(float const*, int, float*)') == 'k_mean'


def test_limits_decide_the_exit_status(capsys):
  assert kr.main(['--log', LOG]) == 0
  out = capsys.readouterr().out.splitlines()
  assert len(out) == 5 and out[0].split()[:4] == ['VGPR', 'AGPR', 'vspill', 'scratch']
  assert kr.main(['--log', LOG, '--match', 'k_igemm', '--max-scratch', '0',
                  '--max-vgpr-spill', '0']) == 0
  assert kr.main(['--log', LOG, '--match', 'k_grouped', '--max-scratch', '0']) == 1
  assert kr.main(['--log', LOG, '--match', 'k_grouped', '--max-vgpr-spill', '49',
                  '--max-scratch', '76']) == 0
  assert kr.main(['--log', LOG, '--match', 'k_grouped', '--max-vgpr-spill', '48']) == 1
  assert kr.main(['--log', LOG, '--match', 'no_such_kernel', '--max-scratch', '0']) == 1
  capsys.readouterr()
