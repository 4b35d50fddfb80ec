------------------------------ MODULE treiber_procs ------------------------------
(* Written to show: A TREIBER-STYLE STACK TOP with push and pop as PROCEDURES, a fair Pusher beside an UNFAIR Popper.  push reads the top and installs its value by compare-and-swap, retrying when the top moved; the Popper pops at most once and may stop anywhere.  The Pusher's conjuncts are WF_vars of its own labels and WF_vars of push's labels (the copy in this process); the Popper has none.  One interference at most: the Pusher's operation ends, PushDone HOLDS. *)
EXTENDS Naturals

(* --algorithm treiber_procs
variables top = 0, popped = 0;

procedure push(v)
variables old = 0;
begin
  rd:  old := top;
  cas: if top = old then
         top := v;
         return;
       else
         goto rd;
       end if;
end procedure

procedure pop()
variables seen = 0;
begin
  prd:  seen := top;
  pcas: if top = seen then
          top := 0;
          popped := seen;
          return;
        else
          goto prd;
        end if;
end procedure

fair process Pusher = 0
begin
  go:   call push(1);
  fin:  skip;
end process

process Popper = 1
begin
  once: call pop();
  rest: skip;
end process

end algorithm *)

PushDone == <>(pc[0] = "Done")
=============================================================================
