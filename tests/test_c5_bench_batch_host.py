"""Host: the batch the C5 GPU tests run (tests/test_gpu_c5_bench_batch.py) is the batch bench.py times.  Read from bench.py's source
with ast: nothing is imported from it or changed."""
import ast
import os

from helpers import ROOT, C5_BENCH_BATCH


def _default_args(path, func):
    tree = ast.parse(open(path).read(), filename=path)
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == func:
            args = node.args.args
            return {a.arg: ast.literal_eval(d) for a, d in zip(args[len(args) - len(node.args.defaults):], node.args.defaults)}
    raise AssertionError(f"{func} not found in {path}")


def test_c5_gpu_tests_run_the_batch_the_bench_times():
    assert _default_args(os.path.join(ROOT, "bench.py"), "c5_bf16")["batch"] == C5_BENCH_BATCH
