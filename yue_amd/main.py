"""Menu front end (reference main.py:7-80).  `python -m yue_amd.main` from the repository root."""
import time

from .tool.config import Config
from .yue import Yue

MENU = {'1': 'BPR', '2': 'FISM', '3': 'WRMF', '4': 'IPF', '5': 'UserKNN', 'a1': 'CUNE', 'a2': 'Song2vec', 'a4': 'CDAE', 'a6': 'ExpoMF', 'a7': 'CoFactor', 'a8': 'LightGCN', 'a9': 'NGCF', 'a10': 'APR'}


def main():
    print('=' * 80)
    print('   Yue: Library for Music Recommendation (MI355X BPR path).   ')
    print('=' * 80)
    print('CF-based Recommenders:')
    print('1. BPR   2. FISM   3. WRMF   4. IPF   5. UserKNN')
    print('Advanced Recommenders:')
    print('a1. CUNE (friends from -net hip or -friends, see recommender/advanced/CUNE.py)')
    print('a2. Song2vec (embedding from -emb hip or -emb FILE.npy, see recommender/advanced/Song2vec.py)')
    print('a4. CDAE   a6. ExpoMF   a7. CoFactor   a8. LightGCN   a9. NGCF   a10. APR')
    print('=' * 80)
    order = input('Please enter the num of the algorithm to run it:')
    start = time.time()
    if order not in MENU:
        print('Error num!')
        exit(-1)
    conf = Config('./config/' + MENU[order] + '.conf')      # the user's own file, as in the reference (main.py:36-37)
    Yue(conf).execute()
    print("Run time: %f s" % (time.time() - start))


if __name__ == '__main__':
    main()
