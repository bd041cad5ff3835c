"""Record the reference's public call signatures as data: tests/golden/ref_signatures.json.

    python tests/golden/make_ref_signatures.py REFERENCE_CHECKOUT [out.json]

SelfPlayAgent / MCTS: parameter lists (name, default as written) of the public methods, read from the .pyx source text (`cpdef`
methods of a `cdef class` carry no introspectable signature).  Coach: the parameter lists and source lines of the five self-play
methods the native adapter replaces, and the order in which learn() calls them.  tests/test_install_conformance.py and
tests/test_iteration_cpu.py hold this package to the record; where the checkout is present they also check the record against it."""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

COACH_FIVE = ['generateSelfPlayAgents', 'processSelfPlayBatches', 'saveIterationSamples', 'processGameResults', 'killSelfPlayAgents']


def coach_record(coach_py):
    """{five: {method: {params, line}}, learn_calls: [...]} of the reference's Coach (Coach.py)"""
    tree = ast.parse(open(coach_py).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'Coach')
    fns = {f.name: f for f in cls.body if isinstance(f, ast.FunctionDef)}
    learn = fns['learn']
    calls = [n.func.attr for n in sorted((n for n in ast.walk(learn) if isinstance(n, ast.Call)), key=lambda n: (n.lineno, n.col_offset))
             if isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == 'self']
    return {'five': {m: {'params': [a.arg for a in fns[m].args.args], 'line': fns[m].lineno} for m in COACH_FIVE},
            'learn_calls': [c for c in sorted(set(calls), key=calls.index) if c in COACH_FIVE]}


def record(ref):
    from test_install_conformance import _ref_signatures
    az = os.path.join(ref, 'alphazero')
    return {'SelfPlayAgent': _ref_signatures(os.path.join(az, 'SelfPlayAgent.pyx'), 'SelfPlayAgent'),
            'MCTS': _ref_signatures(os.path.join(az, 'MCTS.pyx'), 'MCTS'),
            'Coach': coach_record(os.path.join(az, 'Coach.py'))}


if __name__ == '__main__':
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'ref_signatures.json')
    with open(out, 'w') as fh:
        json.dump(record(sys.argv[1]), fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', out)
