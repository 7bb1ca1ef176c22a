"""CPU: what tests/member_rows.py hands the four plan-level suites.  The digests are those of the tensors the suites generated when
each carried a generator of its own (SHA-256 over the bytes of x, dy, w, mu1, mu2; numpy's RandomState stream does not change between
versions), the tuples the literal lists they parametrised over: a change to the shared module that moves a suite's data or its test
ids fails here, without a device."""
import hashlib

import pytest

import member_rows as mr

RAND = {        # x ~ U[0, 1): every row
    "split_17x13_m2": "910af4ed79ad27c5687accb4b61f440957644b1a52ccbff283875ebc16ef30cd",
    "split_17x13_m3": "5cb72b5508a862a1869be6b33b8266c9c4eaeae1164d96757d61c21ad55c53e5",
    "split_17x13_m4": "3e76ce8489b981ea6c1925c4d14cb2c7315aa71b96f17106044a3b85ba3355c1",
    "split_9x70_m2": "7a412d4b25229e3fb6ef3b1da94e9f394eaf59c515713de5973c1abd95a13b9e",
    "split_9x70_m3": "d9bd06327460b833a251ed9b8754a4a651349731d7d65b173b37f73261311886",
    "split_9x70_m4": "fb4f8485d2d04f2ca361a385e74f5bf7268be579ce1761b782dcdce909ba39ef",
    "split_tall_28x28": "eef652dc2dba6fe641e719fad502e9b89c793b35faa7c6afd451a112b606f350",
    "outliers_28x28": "e690fe524404c846fe749ab5ed6c49ec8e734ae21ba198d8c0f3e851f2ac17ed",
    "exact_stacked_28x28": "906e74b1f7fed39b7efd42a9d368cba56da076d504de4e101352ef87ba7027f1",
    "exact_bucket8": "718b2f083846be7658930980ecfdab7cfcf2b6af2195807594de9e9bef6d082e",
    "k65_33x20": "80c92421c7721417c1e63eec499c581c25b0753e50efa0ea336455cd8109811d",
    "k65_gather_windows": "611ad4934c311d6a3b150450bdabe82f0ddba23227f7e796a9f0ecc640f5e06d",
    "unit_testing_24x24": "d8a0c94e8ea7a697067a986a104f802e15c866f4489b6ac5d761129ea3e734b4",
    "unit_testing_32x32": "da1a4677ce9352324fc47b2f60d3dc0b547b9e5f1ebc6965aaec88bfde42505a",
    "single_dim": "42df0d13e31dad30dc3e078de4f970c09bd47ec22f75462ff59b90e9af6d1d23",
    "default_128": "9d4aa486abe3421fb1ca23d7edd5d8988145c05554408b93cdba87ce93180e7f",
    "split_tall_28x28_n4": "c12a379cd31f5bd322a9a83e388aa32062ac4ee1034e5a8a366e46e8e07ca91a",
}
RANDN = {       # x ~ N(0, 1): the rows of test_gpu_input_relu.py
    "split_17x13_m2": "a281736ee9ecd555d58275e2e9a7b60543d1bdf7c97e3d837ce230b4b4ed45d1",
    "split_17x13_m3": "732381b98026bb47a3aef19a1c6b8093d209e7ca47dc2910c082d574b0e14455",
    "split_17x13_m4": "179c519ed4fc3f86a0a79b04fad964547c0a8dd9ddf95e1a2566915c1466ff3a",
    "split_tall_28x28": "1639c9022187f58749b4afbe060e9737fbf04d8455b0c2f2a43707df033471d7",
    "outliers_28x28": "5370e2438d711a70cb4f13ac16cb363e3f40ac5c5598eea2189f748c48b6090b",
    "exact_stacked_28x28": "d450ef42e83e938bc0504cf30ad00ab90ecc9f2ea86695038e5847e5e18dad80",
    "exact_bucket8": "ea6f2383f6abc7d43cc6610c47ebae8cfed5fe61e4ff40221ccaad2ad99eb340",
    "k65_gather_windows": "ef0106c8c22c61aad7aaf9c61cda00e1811c43a3e135a2b9c9e6a20626c8e037",
    "default_128": "17cf23c8b697a21d04b71e92475788d73567e7715cce94fdc39995f2bb7aba3e",
    "split_tall_28x28_n4": "f48234f73d7f671a79cca69a3c1e3ed3b2dd8b493d26789397a596b8c032a707",
}


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def test_every_row_has_its_digest():
    assert set(RAND) == set(mr.ROWS) and len(mr.ROWS) == 17
    assert set(RANDN) == set(mr.FUSED_ROWS) | set(mr.SLAB_ROWS.values())


@pytest.mark.parametrize("x, want", [("rand", RAND), ("randn", RANDN)], ids=["rand", "randn"])
def test_generated_tensors_are_the_ones_the_suites_always_had(x, want):
    for name in want:
        assert _digest(mr.inputs(name, x)) == want[name], name


def test_suites_parametrise_over_the_lists_they_had():
    assert list(mr.FUSED_ROWS) == ["split_17x13_m2", "split_17x13_m3", "split_17x13_m4", "split_tall_28x28", "outliers_28x28",
                                   "exact_stacked_28x28", "exact_bucket8", "k65_gather_windows", "default_128"]
    assert list(mr.NHWC_ROWS) == ["split_17x13_m2", "split_17x13_m3", "split_17x13_m4", "split_9x70_m2", "split_9x70_m3", "split_9x70_m4",
                                  "split_tall_28x28", "outliers_28x28", "exact_stacked_28x28", "exact_bucket8", "k65_33x20",
                                  "k65_gather_windows", "unit_testing_24x24", "unit_testing_32x32", "single_dim", "default_128"]
    assert mr.SLAB_ROWS == {"exact_stacked_28x28": "exact_stacked_28x28", "split_tall_28x28": "split_tall_28x28_n4"}
    for names in (mr.FUSED_ROWS, mr.NHWC_ROWS, mr.SLAB_ROWS.values()):
        assert set(names) <= set(mr.ROWS)
