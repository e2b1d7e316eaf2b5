"""Every entry point of include/magpo.h is called by name in some GPU test module, or is listed here with the test that reaches it
through a host wrapper (the product's, or the one helper shared by the GPU modules in tests/gpu_util.py).  A new entry point without a primitive test fails this module on the CPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# entry points no GPU module calls by name: the test (module::function) that reaches each through the product's host code
INDIRECT = {
    "magpo_last_error": "tests.test_row_kernels_gpu::test_obsnorm_rejects_bad_arguments",          # _Lib.call reads it on every error status
    "magpo_abi_version": "tests.test_abi::test_host_entry_points_without_gpu",
    "magpo_key_split_host": "tests.test_abi::test_host_entry_points_without_gpu",
    "magpo_random_bits_host": "tests.test_abi::test_host_entry_points_without_gpu",
    "magpo_key_fold_in_host": "tests.test_actor_torso::test_init_from_key_matches_restatement",     # params._fold_in
    "magpo_lbf_reset": "tests.test_lbf_gpu::test_lbf_env_matches_oracle",                           # LbfEnvBatch
    "magpo_lbf_step": "tests.test_lbf_gpu::test_lbf_env_matches_oracle",
    "magpo_rware_layout": "tests.test_rware_gpu::test_rware_env_matches_oracle",                    # RwareEnvBatch
    "magpo_rware_reset": "tests.test_rware_gpu::test_rware_env_matches_oracle",
    "magpo_rware_step": "tests.test_rware_gpu::test_rware_env_matches_oracle",
    "magpo_connector_reset": "tests.test_connector_gpu::test_connector_env_matches_restatement",    # ConnectorEnvBatch
    "magpo_connector_step": "tests.test_connector_gpu::test_connector_env_matches_restatement",
    "magpo_mpe_reset": "tests.test_mpe_gpu::test_mpe_env_matches_restatement",                      # MpeEnvBatch
    "magpo_mpe_step": "tests.test_mpe_gpu::test_mpe_env_matches_restatement",
    "magpo_sable_act": "tests.test_act_instances_gpu::test_forced_instance_equals_kernel_composition_under_graph_replay",   # SableGuider.act_fused
    "magpo_act_weight_layout": "tests.test_act_instances_gpu::test_forced_instance_equals_kernel_composition_under_graph_replay",   # SableGuider.refresh
    "magpo_transpose_pad": "tests.test_kernels_gpu::test_linear_shared_tile",                      # tests.gpu_util.transpose_pad (exactness asserted there)
}


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magpo.h")).read(), flags=re.S)
    return re.findall(r"^\s*(?:const char\*|int|long)\s+(magpo_\w+)\s*\(", text, flags=re.M)


def test_every_entry_point_has_a_test():
    names = _declared()
    assert len(names) >= 70 and len(set(names)) == len(names)
    gpu_src = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*_gpu.py"))))
    direct = {n for n in names if f'"{n}"' in gpu_src}
    missing = [n for n in names if n not in direct and n not in INDIRECT]
    assert not missing, f"entry points of include/magpo.h that no GPU test calls and the indirect list does not name: {missing}"
    stale = [n for n in INDIRECT if n not in names or n in direct]
    assert not stale, f"indirect entries that are not declared any more, or are called directly now: {stale}"


def test_indirect_entries_name_existing_tests():
    for name, ref in INDIRECT.items():
        mod, fn = ref.split("::")
        path = os.path.join(ROOT, *mod.split(".")) + ".py"
        assert os.path.exists(path), (name, ref)
        assert re.search(rf"^def {re.escape(fn)}\(", open(path).read(), flags=re.M), (name, ref)
