"""rocprofv3 kernel name -> the library's launch label (cxrk_last_launch_label, the keys of bench.py's roofline table); shared by
pmc_summary.py and pmc_sq_summary.py."""
import re


def key(k):
    if "conv3x3_wgrad_window_kernel" in k:      # csrc/conv_halo_wgrad.h
        return "conv3x3_wgrad_window_kernel"
    m = re.search(r"conv3x3_halo_kernel<.*,\s*(?:\(bool\))?(true|false|1|0)\s*>", k)   # csrc/conv_halo.h: <filter loader, DGRAD>
    if m:
        return f"conv3x3_halo_kernel<{'dgrad' if m.group(1) in ('true', '1') else 'fwd'}>"
    m = re.search(r"gemm_pw_kernel<cxrk::PwCfg<(\d), (\d), (\d)>, cxrk::(\w+)<[^>]*>, cxrk::(\w+)<[^>]*>\s*>", k)
    if m:
        cfg = {"244": "Pw256", "222": "Pw128", "412": "Pw256x64", "142": "Pw64x256"}.get(m.group(1) + m.group(2) + m.group(3), "Pw?")
        return f"gemm_pw_kernel<{cfg},{m.group(4)},{m.group(5)}>"
    m = re.search(r"(gemm_x3_kernel)<cxrk::(\w+)<\d+, cxrk::PL[^>]*>, cxrk::(\w+)<\d+, cxrk::PL[^>]*>\s*, (\d), (\d)\s*>", k)
    if m:
        return f"{m.group(1)}<{m.group(2)}<PL>,{m.group(3)}<PL>,{m.group(4)},{m.group(5)}>"
    m = re.search(r"(gemm_\w+_kernel)<cxrk::(\w+)<[^>]*>, cxrk::(\w+)<[^>]*>\s*(?:, (\d), (\d))?\s*>", k)
    if m:
        return f"{m.group(1)}<{m.group(2)},{m.group(3)}" + (f",{m.group(4)},{m.group(5)}>" if m.group(4) else ">")
    return re.sub(r"\(.*", "", k.replace("(anonymous namespace)::", "")).replace("void ", "").replace("cxrk::", "")[:50]
