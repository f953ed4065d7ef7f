#!/usr/bin/env python3
"""What the compiler made of every kernel instantiation of libnexoclom_hip.so, without a GPU.

Compiles csrc/nxc_api.hip device-only with the flags of nexoclom_amd/build.py plus
``-S -Rpass-analysis=kernel-resource-usage`` into a temporary directory and writes one JSON object
per kernel, keyed by its mangled name: SGPRs, VGPRs, AGPRs, scratch, spills, LDS, occupancy, the
number of instructions, and a hash of the instruction stream with comments, directives and the
numbers of the basic-block labels removed.  The hash is an identity of the whole stream: equal
hashes mean the kernel compiled to the same instructions.

    python tools/kernel_resources.py --out profiles/kernel_resources.json
    python tools/kernel_resources.py --source OTHER_TREE/nexoclom_amd/csrc/nxc_api.hip --out other.json
    python tools/kernel_resources.py --against other.json      # every instantiation that differs, and how
"""
import argparse
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build():
    # by path: importing the package would load the built library
    spec = importlib.util.spec_from_file_location(
        'nxc_build', os.path.join(ROOT, 'nexoclom_amd', 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REMARK = re.compile(r'remark:\s+(.*?):\s+(.*?)(?:\s+\[-Rpass-analysis=[^\]]*\])?$')
FIELDS = {'SGPRs': 'sgprs', 'TotalSGPRs': 'sgprs', 'VGPRs': 'vgprs', 'AGPRs': 'agprs',
          'ScratchSize [bytes/lane]': 'scratch_bytes_per_lane', 'Dynamic Stack': 'dynamic_stack',
          'Occupancy [waves/SIMD]': 'occupancy_waves_per_simd', 'SGPRs Spill': 'sgpr_spills',
          'VGPRs Spill': 'vgpr_spills', 'LDS Size [bytes/block]': 'lds_bytes_per_block'}


def parse_remarks(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == 'Function Name':
            cur = out.setdefault(val, {})
        elif cur is not None and key in FIELDS:
            cur[FIELDS[key]] = (val == 'True') if val in ('True', 'False') else int(val)
    return out


LABEL = re.compile(r'\.L[A-Za-z_$]*\d+(?:_\d+)?')


def parse_streams(asm):
    """{function: (instruction count, sha256 of the normalised stream)}"""
    out, name, lines, labels = {}, None, [], {}

    def canon(m):
        return labels.setdefault(m.group(0), 'L%d' % len(labels))

    for raw in asm.splitlines():
        line = raw.split(';', 1)[0].strip()
        if name is None:
            m = re.match(r'([A-Za-z_][\w$.]*):$', line)
            if m and not line.startswith('.L'):
                name, lines, labels = m.group(1), [], {}
            continue
        if line.startswith('.Lfunc_end'):
            body = '\n'.join(lines)
            count = sum(1 for ln in lines if not ln.endswith(':'))
            out[name] = (count, hashlib.sha256(body.encode()).hexdigest())
            name = None
            continue
        if not line:
            continue
        if line.startswith('.') and not line.endswith(':'):
            continue                                   # a directive
        lines.append(' '.join(LABEL.sub(canon, line).split()))
    return out


def measure(source):
    build = load_build()
    flags = [f for f in build.FLAGS if f != '-shared']
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'nxc_api.s')
        cmd = [build.hipcc()] + flags + ['--cuda-device-only', '-S',
                                         '-Rpass-analysis=kernel-resource-usage', source, '-o', asm]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stdout + res.stderr)
            raise SystemExit('hipcc failed')
        with open(asm) as f:
            streams = parse_streams(f.read())
    kernels = parse_remarks(res.stderr)
    for name, k in kernels.items():
        k['instructions'], k['stream_sha256'] = streams[name]
    return kernels


def compare(new, old):
    """Lines that say which instantiations differ and how; empty when none does."""
    lines = []
    for name in sorted(set(new) | set(old)):
        a, b = old.get(name), new.get(name)
        if a is None or b is None:
            lines.append('%s: only in %s' % (name, 'this tree' if a is None else 'the other file'))
            continue
        diff = ['%s %s -> %s' % (k, a.get(k), b.get(k)) for k in sorted(set(a) | set(b))
                if k != 'stream_sha256' and a.get(k) != b.get(k)]
        if a.get('stream_sha256') != b.get('stream_sha256'):
            diff.append('instruction stream differs')
        if diff:
            lines.append('%s: %s' % (name, ', '.join(diff)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--source', default=None, help='another nxc_api.hip (default: this tree\'s)')
    ap.add_argument('--out', default=None, help='write the JSON here instead of standard output')
    ap.add_argument('--against', default=None, metavar='FILE',
                    help='print every instantiation that differs from FILE, and how')
    args = ap.parse_args()
    kernels = measure(args.source or load_build().SRC)
    text = json.dumps(kernels, indent=1, sort_keys=True) + '\n'
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text)
    elif not args.against:
        sys.stdout.write(text)
    if args.against:
        with open(args.against) as f:
            lines = compare(kernels, json.load(f))
        print('\n'.join(lines) if lines else 'no kernel differs')
        print('%d of %d instantiations differ' % (len(lines), len(kernels)))


if __name__ == '__main__':
    main()
