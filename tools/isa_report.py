# -*- coding: utf-8 -*-
"""Static report of the compiled kernels (no GPU needed): compiles every translation unit of
ssqueezepy_amd/csrc for gfx950 to assembly and prints, per kernel, registers, scratch (spills),
static LDS, code size and the instruction mix.
    python tools/isa_report.py [substring-filter] [--dump DIR] > profiles/rNN_isa_report.txt
--dump DIR also writes every kernel's normalised body (comments stripped, local labels and mangled symbols
replaced by fixed tokens) to DIR/<unit>/<demangled name>.s: two checkouts compare with `diff -r`."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ssqueezepy_amd', 'csrc')
HIPCC = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')
sys.path.insert(0, ROOT)
from ssqueezepy_amd.build import SOURCES, COMMON       # noqa: E402


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout
    return out.split('\n')


def normalised(body):
    """A kernel's instructions without what differs between two builds of the same code: comments, the
    numbering of local labels, the mangled names of kernels and their LDS arrays."""
    out = []
    for line in body.split('\n'):
        line = re.sub(r'\.L\w+', '.L', re.sub(r'\b_Z\w+', 'SYM', line.split(';')[0])).rstrip()
        if line.strip():
            out.append(line)
    return '\n'.join(out) + '\n'


def main(flt='', dump=None):
    rows, bodies = [], {}
    for src, extra in SOURCES:
        with tempfile.TemporaryDirectory() as td:
            asm = os.path.join(td, 'k.s')
            cmd = [HIPCC] + [c for c in COMMON if c != '-fPIC'] + extra + [
                '-S', '--cuda-device-only', os.path.join(CSRC, src), '-o', asm]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode:
                print(r.stderr[-2000:]); raise SystemExit(1)
            text = open(asm).read()
        meta = {}
        for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', text, re.S):
            name, body = m.group(1), m.group(2)
            get = lambda k: int(re.search(r'\.%s (\d+)' % k, body).group(1)) if re.search(r'\.%s (\d+)' % k, body) else 0
            meta[name] = dict(ldsb=get('amdhsa_group_segment_fixed_size'), scratch=get('amdhsa_private_segment_fixed_size'))
        for m in re.finditer(r'\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)', text):
            if m.group(1) in meta:
                meta[m.group(1)].update(sgpr=int(m.group(2)), vgpr=int(m.group(3)))
        for name in meta:
            b = re.search(r'^%s:[^\n]*\n(.*?)s_endpgm' % re.escape(name), text, re.S | re.M)
            ins = re.findall(r'^\s+([a-z][a-z0-9_]+)', b.group(1), re.M) if b else []
            mix = dict(valu=sum(i.startswith('v_') for i in ins), salu=sum(i.startswith('s_') for i in ins),
                       lds=sum(i.startswith('ds_') for i in ins),
                       vmem=sum(i.startswith(('global_', 'buffer_', 'flat_', 'scratch_')) for i in ins))
            meta[name].update(mix, n=len(ins))
            full = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(name), text, re.S | re.M)
            bodies[name] = full.group(1) if full else ''
            rows.append((src, name, meta[name]))
    names = demangle([r[1] for r in rows])
    print('%-22s %5s %5s %7s %7s %7s | %6s %6s %5s %5s  kernel' %
          ('file', 'vgpr', 'sgpr', 'scratch', 'ldsB', 'instrs', 'valu', 'salu', 'lds', 'vmem'))
    for (src, name, d), dn in zip(rows, names):
        short = re.sub(r'\(.*', '', dn).replace('ssq::', '')
        if flt and flt not in short:
            continue
        if dump:
            os.makedirs(os.path.join(dump, src), exist_ok=True)
            with open(os.path.join(dump, src, re.sub(r'[^\w<>,.-]', '_', short)[:200] + '.s'), 'w') as fh:
                fh.write(normalised(bodies[name]))
        print('%-22s %5d %5d %7d %7d %7d | %6d %6d %5d %5d  %s' %
              (src, d.get('vgpr', 0), d.get('sgpr', 0), d['scratch'], d['ldsb'], d.get('n', 0),
               d.get('valu', 0), d.get('salu', 0), d.get('lds', 0), d.get('vmem', 0), short[:110]))


if __name__ == '__main__':
    args = sys.argv[1:]
    dump = args.pop(args.index('--dump') + 1) if '--dump' in args else None
    args = [a for a in args if a != '--dump']
    main(args[0] if args else '', dump)
