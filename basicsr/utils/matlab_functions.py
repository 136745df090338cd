from codeformer_amd.utils.matlab_functions import *  # noqa: F401,F403
