"""Write tests/golden/train_trace.json (digest, calls per entry point and pointer count of every case of tests/train_trace.py), or
with --dump DIR the full traces, one call per line, for a diff by hand:

    python tools/gen_train_trace.py --dump /tmp/before       # on the commit that passes
    python tools/gen_train_trace.py --dump /tmp/after        # on the one that does not
    diff /tmp/before/300p2-default.jsonl /tmp/after/300p2-default.jsonl

Needs the built library, no device.  The golden is recorded once, from the commit BEFORE a restructuring of ctdet/train_engine.py;
it is regenerated only by a change that means to launch something else.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'context-transformer_amd'), os.path.join(REPO, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

torch.set_num_threads(8)

import train_trace  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dump', metavar='DIR', default=None, help='write full traces here instead of the golden')
    ap.add_argument('--case', action='append', default=None, help='only these case ids (with --dump)')
    args = ap.parse_args()
    out = {}
    for case in train_trace.CASES:
        if args.case and case[0] not in args.case:
            continue
        log, pointers, unnamed = train_trace.trace(case[1], case[2], case[3], os.environ.__setitem__,
                                                   lambda k: os.environ.pop(k, None))
        if unnamed:
            raise SystemExit('%s: pointer arguments outside every named tensor: %s' % (case[0], sorted(set(unnamed))))
        out[case[0]] = train_trace.summary(log, pointers)
        print(case[0], len(log), 'calls', pointers, 'pointers', out[case[0]]['sha256'][:16])
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, case[0] + '.jsonl'), 'w') as f:
                f.writelines(train_trace.canonical(e) + '\n' for e in log)
    if not args.dump:
        with open(os.path.join(REPO, 'tests', 'golden', 'train_trace.json'), 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


if __name__ == '__main__':
    main()
