"""Writes tests/golden/conv_plan.json: the launch plan (dsl_conv2d_plan) of every descriptor of tests/conv_plan_cases.py under every
forced (tile row, split-K factor, workspace) variant, as answered by a GIVEN library.  The committed fixture was written from the
library as it was before the tile-table refactor of csrc/conv.hip (that build's dsl_conv2d given an out-parameter that returns
the numbers just before the launch); regenerate it only from a library whose plans are meant to be the new truth.
Usage (no GPU needed): python tools/gen_conv_plan_golden.py path/to/libdsl_hip.so [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ['DSL_HIP_LIB'] = os.path.abspath(sys.argv[1])
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import conv_plan_cases as P  # noqa: E402

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'conv_plan.json')
doc = dict(fields=P.PLAN_FIELDS, variants=[list(v) for v in P.variants()],
           plans={name: [P.plan(d, *v) for v in P.variants()] for name, d in P.cases().items()})
with open(out, 'w') as f:
    f.write('{"fields": %s,\n "variants": %s,\n "plans": {\n' % (json.dumps(doc['fields']), json.dumps(doc['variants'])))
    f.write(',\n'.join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in doc['plans'].items()))
    f.write('\n }}\n')
print(out, len(doc['plans']), 'descriptors x', len(doc['variants']), 'variants')
