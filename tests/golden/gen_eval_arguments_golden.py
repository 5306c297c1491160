#!/usr/bin/env python3
"""Golden record of the reference's eval/eval_arguments.py (EvalArguments, a dataclass subclass of lightretriever.inference.arguments
.InferenceArguments) parsing the flags of eval/call_evaluate_mteb.sh + the model flags of the launch scripts, made by running the REAL
reference on its own package: the flags, the names of the base-class fields and of the fields EvalArguments adds, and every field's value
after __post_init__.  Build container only (needs a reference checkout).
Usage: PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_eval_arguments_golden.py <reference checkout>"""
import dataclasses
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

ARGV = ["--model_name_or_path", "results/lightretriever-llama3.2-1b", "--benchmark_name", "BEIR", "--top_k", "1000", "--inference_arch",
        "PytorchRPCExactSearchModel", "--output_dir", "/tmp/out", "--batch_size", "256", "--corpus_chunk_size", "100000",
        "--model_type", "HybridModel", "--hybrid_use_emb_vector", "--noncontextual_query_embedding", "--lowercase", "--add_sep_token", "--pooling_strategy",
        "lasttoken", "--score_function", "cos_sim", "--q_max_len", "512", "--p_max_len", "512", "--bf16"]


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "src"))
    from transformers import HfArgumentParser
    import lightretriever.inference.arguments as base
    assert os.path.abspath(base.__file__).startswith(os.path.abspath(ref_root)), base.__file__
    spec = importlib.util.spec_from_file_location("ref_eval_arguments", os.path.join(ref_root, "eval", "eval_arguments.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (a,) = HfArgumentParser(mod.EvalArguments).parse_args_into_dataclasses(ARGV)
    base_fields = [f.name for f in dataclasses.fields(base.InferenceArguments)]
    parsed = {f.name: getattr(a, f.name) for f in dataclasses.fields(a)}
    assert all(v is None or isinstance(v, (bool, int, float, str, list)) for v in parsed.values()), parsed
    out = {"argv": ARGV, "base_fields": base_fields, "eval_fields": [n for n in parsed if n not in base_fields], "parsed": parsed}
    with open(os.path.join(HERE, "eval_arguments.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote eval_arguments.json: %d base fields, eval fields %s" % (len(base_fields), out["eval_fields"]))


if __name__ == "__main__":
    main(sys.argv[1])
