"""The committed seeds and per-family case counts of the forms soak's suite slice: shared by test_gpu_soak_forms.py, which
runs them on the device, and test_soak_forms_cpu.py, which checks that the generators still reach every edge class at
these counts.  profiles/round17/README.md records the timing the counts were chosen by."""
SEEDS = (20261021, 7)
CASES = {"lists": 40, "combine": 40, "frame": 40, "layout": 40, "logread": 40, "logwrite": 40, "sstread": 40,
         "sstwrite": 40, "sequence": 12,
         "captured": 12}
