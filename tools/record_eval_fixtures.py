#!/usr/bin/env python3
"""Record the two fixtures that pin the evaluation side, from a checkout of the commit to record from.

    python tools/record_eval_fixtures.py rows   TREE [--out tests/golden/g12_row_kernels.npz]     (needs the MI355X)
    python tools/record_eval_fixtures.py dropin TREE [--out tests/golden/g13_dropin_eval.npz]     (CPU)

TREE is a built checkout of this repository (e.g. `git worktree add ../parent HEAD~1`, then its build.py): `dmf`, `solver` and
`utils` are imported from TREE, the case builders (tests/row_cases.py, tests/dropin_eval_case.py) from the tree this script
lies in — the same functions the tests run on the tree under test.
  rows    the SHA-256 of every output of dmf_softmax_stats, dmf_prob_scatter and dmf_logits_mean on tests/row_cases.py
  dropin  the decoded artefacts of a drop-in test() + color() with every evaluation key on, and torch's RNG state after them
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('what', choices=['rows', 'dropin'])
    ap.add_argument('tree')
    ap.add_argument('--out')
    ap.add_argument('--commit', help='the commit of TREE, where TREE is an export without its .git')
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(tree, 'dual-modal-fusion_amd'), tree, os.path.join(HERE, 'tests')]
    import dmf
    assert os.path.dirname(os.path.dirname(os.path.abspath(dmf.__file__))) == os.path.join(tree, 'dual-modal-fusion_amd'), dmf.__file__
    git = subprocess.run(['git', '-C', tree, 'rev-parse', 'HEAD'], capture_output=True, text=True)
    commit = args.commit or (git.stdout.strip() if git.returncode == 0 else 'unknown')
    golden = os.path.join(HERE, 'tests', 'golden')
    if args.what == 'rows':
        import row_cases
        arrays = row_cases.pack(row_cases.outputs())
        arrays['seed'] = np.array(row_cases.SEED)
        out = args.out or os.path.join(golden, 'g12_row_kernels.npz')
    else:
        import dropin_eval_case
        with tempfile.TemporaryDirectory(prefix='dmf_record_') as tmp:
            arrays = dropin_eval_case.outputs(golden, tmp)
        out = args.out or os.path.join(golden, 'g13_dropin_eval.npz')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, recorded_from=np.array(commit), **arrays)
    print('%s: %d arrays from %s (%s), %d bytes' % (out, len(arrays), tree, commit, os.path.getsize(out)))


if __name__ == '__main__':
    main()
