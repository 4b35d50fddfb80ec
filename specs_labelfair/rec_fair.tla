------------------------------ MODULE rec_fair ------------------------------
(* Written to show: A RECURSIVE PROCEDURE UNDER `fair`: down calls itself; its one copy in the process keeps a bounded stack.  The Walker's conjuncts are WF_vars of its own labels and WF_vars of down's labels, whichever frame runs them.  Termination HOLDS. *)
EXTENDS Naturals

(* --algorithm rec_fair
variables total = 0;

procedure down(n)
begin
  d1: if n = 0 then
        return;
      else
        total := total + n;
        call down(n - 1);
      end if;
  d2: return;
end procedure

fair process Walker = 0
begin
  w: call down(2);
  e: skip;
end process

end algorithm *)

=============================================================================
