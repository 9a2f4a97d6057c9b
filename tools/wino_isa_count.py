#!/usr/bin/env python
"""Static instruction counts of the fp32 Winograd kernels from a device assembly listing (no GPU needed):

    hipcc -x hip --offload-arch=gfx950 -O3 -std=c++17 -fno-gpu-rdc -Ilatentfusion_amd/csrc --cuda-device-only -S \
          latentfusion_amd/csrc/conv_wino.hip -o wino.s
    python tools/wino_isa_count.py wino.s [more.s ...]
    python tools/wino_isa_count.py --same-as parent.s wino.s     (also: which kernels of parent.s have the same listing in wino.s)

Per kernel: VALU and MFMA instructions, packed / scalar fp32 adds and subtractions, s_nop, VGPRs, spills, scratch.  The
four z-frequency instantiations of wino_compute each run on one wave, so a count / 4 is per wave and tile (plus the
per-launch prologue).  profiles/wino_pack_isa.txt is this tool's output for the parent and the packed form.
conv_wino.hip is the one translation unit of these kernels (wino16_math.h, wino16_compute.h and the two wino16_proj*.inc
next to it are included by it); the comment at wino_epi_* in csrc/wino16_math.h reads the pinned epilogue roundings off this listing."""
import re
import sys

COLS = ('VALU', 'MFMA', 'v_pk_add_f32', 'v_sub_f32', 'v_add_f32', 's_nop', 'nop states', 'VGPR', 'VGPR spill', 'scratch B')


def kernels(path):
    name, rows = None, {}
    for line in open(path):
        t = line.strip()
        m = re.match(r'^(_ZN\S*conv3d_c16_wino\S*):', t)
        if m:
            name = m.group(1)
            rows[name] = dict.fromkeys(COLS, 0)
            continue
        if name is None:
            continue
        if t.startswith('.end_amdhsa_kernel') or t.startswith('.Lfunc_end'):
            if t.startswith('.Lfunc_end'):
                name = None
            continue
        r = rows[name]
        op = t.split()[0] if t and not t.startswith((';', '.')) else ''
        if op.startswith('v_mfma'):
            r['MFMA'] += 1
        elif op.startswith('v_') and not op.startswith('v_nop'):
            r['VALU'] += 1
        if op == 'v_pk_add_f32':
            r['v_pk_add_f32'] += 1
        elif op.startswith('v_sub_f32') or op.startswith('v_subrev_f32'):
            r['v_sub_f32'] += 1
        elif op.startswith('v_add_f32'):
            r['v_add_f32'] += 1
        elif op == 's_nop':
            r['s_nop'] += 1
            r['nop states'] += int(t.split()[1]) + 1
    # resource lines of the kernel descriptors / metadata
    text = open(path).read()
    for name, r in rows.items():
        m = re.search(r'\.amdhsa_kernel %s\b(.*?)\.end_amdhsa_kernel' % re.escape(name), text, re.S)
        if m:
            g = re.search(r'\.amdhsa_next_free_vgpr (\d+)', m.group(1))
            s = re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', m.group(1))
            r['VGPR'] = int(g.group(1)) if g else -1
            r['scratch B'] = int(s.group(1)) if s else -1
        m = re.search(r'\.name:\s+%s\b.*?\.vgpr_spill_count:\s+(\d+)' % re.escape(name), text, re.S)
        r['VGPR spill'] = int(m.group(1)) if m else -1
    return rows


FORMS = {'1': 'fwd block', '2': 'dgrad+prev', '3': 'dgrad plain'}


def short(name):
    m = re.search(r'(conv3d_c16_wino\w*?_form_kernel)ILi(\d)ELi(\d)E', name)
    if m:                                                       # the fixed epilogue forms: <form, OPT>
        return f'{m.group(1)}<{FORMS[m.group(2)]}, {m.group(3)}>'
    m = re.search(r'(conv3d_c16_wino\w*?_kernel)(ILb([01])E)?', name)
    return m.group(1) + ({'1': '<packed>', '0': '<scalar>', None: ''}[m.group(3)])


def listings(path):
    """Per kernel: its instructions and labels, comments dropped, the function's index taken out of the block labels."""
    name, out = None, {}
    for line in open(path):
        t = line.strip()
        m = re.match(r'^(_ZN\S*conv3d_c16_wino\S*):', t)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and t.startswith('.Lfunc_end'):
            name = None
        elif name is not None:
            t = re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r';.*', '', t)).strip()
            if t:
                out[name].append(t)
    return out


args = sys.argv[1:]
base = None
if args[:1] == ['--same-as']:
    base, args = args[1], args[2:]
for path in args:
    print(f'# {path}')
    print('| kernel | ' + ' | '.join(COLS) + ' |')
    print('|---|' + '---|' * len(COLS))
    for name, r in kernels(path).items():
        print(f'| `{short(name)}` | ' + ' | '.join(str(r[c]) for c in COLS) + ' |')
    if base is not None:
        old, new = listings(base), listings(path)
        print(f'\n# listings of {base} against {path} (comments dropped, block labels renumbered):')
        for name, body in old.items():
            print(f'#   `{short(name)}`: {len(body)} lines, ' + ('IDENTICAL' if new.get(name) == body else 'DIFFERENT' if name in new else 'absent'))
