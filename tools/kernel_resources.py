"""Per-kernel register / scratch / LDS figures of the HIP sources, from the compiler's
resource-usage remarks (-Rpass-analysis=kernel-resource-usage), one row per kernel.

  python tools/kernel_resources.py                      # compile the product sources, print all
  python tools/kernel_resources.py --sources dopamine_amd/csrc/nature_cnn.hip --match k_grouped
  python tools/kernel_resources.py --log remarks.log    # a recorded remark log instead
  ... --match 'PairOp' --max-scratch 0 --max-vgpr-spill 0   # exit 1 if a matching kernel exceeds

The sources are compiled with _build's product flags (device code only, objects discarded).
Only the remark's numbers are read: nothing here looks at instructions.  A grouped kernel's
row names its ops in launch order, each shortened to its template heads, e.g.
  k_grouped<1024: Rider | Gemm<1,1,16 DyT,Im2colT,EpiPartial> | Pair<Gemm<1,1,8 SubPixDy<0,0>,...>> ...>
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

_FIELDS = {
    'TotalSGPRs': 'sgprs', 'VGPRs': 'vgprs', 'AGPRs': 'agprs',
    'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'occupancy',
    'SGPRs Spill': 'sgpr_spill', 'VGPRs Spill': 'vgpr_spill', 'LDS Size [bytes/block]': 'lds',
}
_REMARK = re.compile(r'remark:\s+(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]')


def parse_remarks(text):
  """[{name (mangled), sgprs, vgprs, agprs, scratch, occupancy, sgpr_spill, vgpr_spill, lds}]
  in the log's order; a kernel that several translation units emit appears once per unit."""
  out, cur = [], None
  for line in text.splitlines():
    m = _REMARK.search(line)
    if not m:
      continue
    body = re.sub(r'^\S+:\d+:\d+:\s*', '', m.group(1))   # 'remark: file:line:col: ...' form
    if body.startswith('Function Name:'):
      cur = {'name': body.split(':', 1)[1].strip()}
      out.append(cur)
      continue
    if cur is None or ':' not in body:
      continue
    key, val = body.rsplit(':', 1)
    key = _FIELDS.get(key.strip())
    if key:
      try:
        cur[key] = int(val)
      except ValueError:
        pass
  return out


def demangle(names):
  """names -> demangled, through llvm-cxxfilt / c++filt when one is there (else unchanged)."""
  for tool in ('llvm-cxxfilt', '/opt/rocm/llvm/bin/llvm-cxxfilt', 'c++filt'):
    try:
      r = subprocess.run([tool], input='\n'.join(names) + '\n', capture_output=True, text=True,
                         check=True)
    except (OSError, subprocess.CalledProcessError):
      continue
    got = r.stdout.splitlines()
    if len(got) == len(names):
      return got
  return list(names)


def _split_args(s):
  """Top-level comma split of a template argument list."""
  out, depth, start = [], 0, 0
  for i, ch in enumerate(s):
    if ch in '<(':
      depth += 1
    elif ch in '>)':
      depth -= 1
    elif ch == ',' and depth == 0:
      out.append(s[start:i].strip())
      start = i + 1
  tail = s[start:].strip()
  if tail:
    out.append(tail)
  return out


def _head_args(s):
  """'ns::Name<args>' -> ('Name', [args]); no template: ('Name', [])."""
  s = s.strip()
  i = s.find('<')
  if i < 0 or not s.endswith('>'):
    return s.split('::')[-1], []
  return s[:i].split('::')[-1], _split_args(s[i + 1:-1])


def _is_value(a):
  return bool(re.fullmatch(r'\(?[\w ]*\)?-?\d+|true|false', a.strip()))


def short_op(s):
  """One op type, shortened: integer arguments kept, class arguments by their heads."""
  name, args = _head_args(s)
  if name == 'PairOp':
    return 'Pair<%s>' % short_op(args[0])
  if name == 'RiderOpT':
    return 'Rider' + ('(groups)' if args and args[0] == 'true' else '')
  if name in ('Conv',):
    return name
  if not args:
    return name
  ints = [a for a in args if _is_value(a)]
  classes = [short_op(a) for a in args if not _is_value(a) and short_op(a) != 'Conv']
  name = name[:-2] if name.endswith('Op') and len(name) > 2 else name
  ints = [re.sub(r'^\(.*\)', '', a) for a in ints]
  parts = ','.join(ints)
  if classes:
    parts += (' ' if parts else '') + ','.join(classes)
  return '%s<%s>' % (name, parts)


def short_kernel(dem):
  """A demangled kernel -> 'k_grouped<T: op | op | ...>' (others: name<shortened args>)."""
  dem = re.sub(r'^void\s+', '', dem.strip())
  dem = re.sub(r'\)\s*(const)?\s*$', ')', dem)
  depth, cut = 0, len(dem)
  for i, ch in enumerate(dem):            # strip the parameter list: the last top-level '('
    if ch == '<':
      depth += 1
    elif ch == '>':
      depth -= 1
    elif ch == '(' and depth == 0:
      cut = i
      break
  name, args = _head_args(dem[:cut])
  if name == 'k_grouped' and args:
    return 'k_grouped<%s: %s>' % (args[0], ' | '.join(short_op(a) for a in args[1:]))
  return short_op(dem[:cut])


def compile_remarks(sources, extra=(), verbose=False):
  """The product flags + the remarks, device code only; returns the compiler's stderr."""
  from dopamine_amd import _build
  csrc = os.path.join(ROOT, 'dopamine_amd', 'csrc')
  flags = ['--offload-arch=' + _build.ARCH, '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off',
           '-I', csrc] + list(_build.PRODUCT_FLAGS) + list(extra) + [
               '-DDQ_BUILD_FLAGS="%s"' % _build.flags_string(_build.PRODUCT_FLAGS),
               '-Rpass-analysis=kernel-resource-usage', '--cuda-device-only', '-c']
  procs = []
  with tempfile.TemporaryDirectory() as tmp:
    for i, src in enumerate(sources):
      cmd = ['hipcc'] + flags + ['-o', os.path.join(tmp, '%d.o' % i), src]
      if verbose:
        print(' '.join(cmd), file=sys.stderr)
      procs.append((subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True), cmd))
    text = ''
    for p, cmd in procs:
      err = p.communicate()[1]
      if p.returncode != 0:
        sys.stderr.write(err)
        raise subprocess.CalledProcessError(p.returncode, cmd)
      text += err
  return text


def rows_of(text):
  recs = parse_remarks(text)
  for r, d in zip(recs, demangle([r['name'] for r in recs])):
    r['demangled'] = d
    r['short'] = short_kernel(d)
  return recs


_COLS = (('vgprs', 'VGPR'), ('agprs', 'AGPR'), ('vgpr_spill', 'vspill'), ('scratch', 'scratch'),
         ('sgprs', 'SGPR'), ('sgpr_spill', 'sspill'), ('lds', 'LDS'), ('occupancy', 'occ'))


def format_rows(recs):
  head = ' '.join('%7s' % h for _, h in _COLS) + '  kernel'
  lines = [head]
  for r in recs:
    lines.append(' '.join('%7s' % r.get(k, '-') for k, _ in _COLS) + '  ' + r['short'])
  return '\n'.join(lines)


def over_limit(recs, max_scratch=None, max_vgpr_spill=None):
  bad = []
  for r in recs:
    if max_scratch is not None and r.get('scratch', 0) > max_scratch:
      bad.append((r, 'scratch %d > %d' % (r['scratch'], max_scratch)))
    elif max_vgpr_spill is not None and r.get('vgpr_spill', 0) > max_vgpr_spill:
      bad.append((r, 'VGPR spills %d > %d' % (r['vgpr_spill'], max_vgpr_spill)))
  return bad


def main(argv=None):
  ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  ap.add_argument('--log', help='read a recorded remark log instead of compiling')
  ap.add_argument('--sources', nargs='*', help='sources to compile (default: the product sources)')
  ap.add_argument('--flag', action='append', default=[], help='an extra compiler flag (repeatable)')
  ap.add_argument('--save-log', help='keep the compiler remarks in this file')
  ap.add_argument('--match', help='regex on the demangled or shortened kernel name')
  ap.add_argument('--max-scratch', type=int, help='fail when a matching kernel has more bytes/lane')
  ap.add_argument('--max-vgpr-spill', type=int, help='fail when a matching kernel spills more VGPRs')
  ap.add_argument('-v', '--verbose', action='store_true')
  a = ap.parse_args(argv)
  if a.log:
    with open(a.log) as f:
      text = f.read()
  else:
    from dopamine_amd import _build
    text = compile_remarks(a.sources or _build.SOURCES, a.flag, a.verbose)
    if a.save_log:
      with open(a.save_log, 'w') as f:
        f.write(text)
  recs = rows_of(text)
  if a.match:
    rx = re.compile(a.match)
    recs = [r for r in recs if rx.search(r['demangled']) or rx.search(r['short'])]
  print(format_rows(recs))
  bad = over_limit(recs, a.max_scratch, a.max_vgpr_spill)
  for r, why in bad:
    print('OVER: %s: %s' % (why, r['short']), file=sys.stderr)
  if (a.max_scratch is not None or a.max_vgpr_spill is not None) and not recs:
    print('OVER: no kernel matches %r' % a.match, file=sys.stderr)
    return 1
  return 1 if bad else 0


if __name__ == '__main__':
  sys.exit(main())
