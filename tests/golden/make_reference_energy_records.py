"""Record what the front end makes of the reference's own example energy files.

The reference's examples/<name>/<name>.t are program text and are not stored here; the
tests that pin our energies/<name>.t to them (tests/test_generic_frontend.py,
tests/test_family_routing.py, tests/test_abi.py) compare against these records instead:
for every example, the SHA-256 of its residual templates as the hash-consed pool prints
them (api.generic_describe), the SHA-256 of its structural signature
(api.generic_signature: declarations, ComputedArrays, exclusion and residuals, names
dropped), the number of templates, the kernel family Opt_ProblemDefine picks for it, and
the solver kinds Opt_ProblemDefine accepts it with. Results only: no text of the files.

    python tests/golden/make_reference_energy_records.py <reference checkout>

writes tests/golden/reference_energies.json (build the library first).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

EXAMPLES = ["arap_mesh_deformation", "cotangent_mesh_smoothing", "embedded_mesh_deformation", "image_warping",
            "intrinsic_image_decomposition", "optical_flow", "poisson_image_editing", "robust_nonrigid_alignment",
            "shape_from_shading", "volumetric_mesh_deformation"]
KINDS = ["gaussNewtonGPU", "LMGPU"]


def sha(text: str) -> str:
    return hashlib.sha256(text.encode()).hexdigest()


def describe_sha(api, path: str) -> str:
    return sha("\n".join(api.generic_describe(path)))


def signature_sha(api, path: str) -> str:
    return sha(api.generic_signature(path))


def defines(api, path: str, kind: str) -> bool:
    lib = api.load_library()
    ip = api.InitParams()
    ip.backend = b"backend_cuda"
    st = lib.Opt_NewState(ip)
    pr = lib.Opt_ProblemDefine(st, path.encode(), kind.encode())
    if pr:
        lib.Opt_ProblemDelete(st, pr)
    return bool(pr)


def main(ref):
    from opt_amd import api

    out = {}
    for name in EXAMPLES:
        path = os.path.join(ref, "examples", name, name + ".t")
        out[name] = {
            "describe_sha256": describe_sha(api, path),
            "signature_sha256": signature_sha(api, path),
            "templates": len(api.generic_describe(path)),
            "family": api.problem_family(path),
            "defines": {k: defines(api, path, k) for k in KINDS},
        }
    dst = os.path.join(HERE, "reference_energies.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(dst)


if __name__ == "__main__":
    main(sys.argv[1])
